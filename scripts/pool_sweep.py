"""Where hop 2's early exit never happens: CAPSMI_HOP2=pool against =cells on tables of uniform in-degree d.

Targets = d copies of a random list of distinct ids out of 2^--log-ids, sources random: no pair finds its target
set before its own group has been seen, so the pool's hop 2 reads X once per relationship (nearly) and needs
every source line.  Per d and mode: the library's event timers per kernel (ms per launch over --steps steps),
the time after pass 1 (every timed kernel but part_scatter1) and the wall time per call.  One JSON document on
stdout, in the form of profiles/r07_pool_sweep.json.

    python scripts/pool_sweep.py --log-ids 26 --d 1,2,4
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "cypher-for-apache-spark_amd")]

KERNELS = ("part_scatter1", "hop1", "hop2", "part_scatter2", "part_scatter2_hop1")


def kernel_times(sess, lib):
    out = {}
    for k in KERNELS:
        cnt, ms = ctypes.c_int64(), ctypes.c_double()
        lib.call("capsmi_session_kernel_time", sess.handle, k.encode(), ctypes.byref(cnt), ctypes.byref(ms))
        if cnt.value:
            out[k] = ms.value / cnt.value
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-ids", type=int, default=26)
    ap.add_argument("--d", default="1,2,4")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--modes", default="pool,cells")
    args = ap.parse_args()
    from capsmi import ColumnData, I64, Session, _lib, graph
    n = 1 << args.log_ids
    sess = Session(0)
    full = graph.NodeBitmap(sess, 0, n).add_scan(graph.rmat_nodes(sess, args.log_ids, graph.NODES_ALL), "id")
    doc = {"ids": n, "steps": args.steps, "tables": []}
    for d in (int(x) for x in args.d.split(",")):
        rng = np.random.default_rng(7 + d)
        t0 = time.perf_counter()
        m = min(d * n, 1 << 28)
        ids = rng.permutation(n)[:m // d].astype(np.int64)
        dst = np.tile(ids, d)
        src = rng.integers(0, n, m, dtype=np.int64)
        rels = sess.table([ColumnData("id", I64, np.arange(m, dtype=np.int64)), ColumnData("source", I64, src),
                           ColumnData("target", I64, dst)])
        row = {"d": d, "m": m, "gen_s": round(time.perf_counter() - t0, 1)}
        del src, dst
        for mode in args.modes.split(","):
            sess.set_config("CAPSMI_HOP2", mode)
            pool0, cells0 = sess.route_count("hop2_pool"), sess.route_count("hop2_cells")
            answer = graph.two_hop_count_distinct(sess, [rels], full, full, full)  # warm-up
            _lib.call("capsmi_session_set_profiling", sess.handle, 1)
            kernel_times(sess, _lib)  # reset
            for _ in range(args.steps):
                graph.two_hop_count_distinct(sess, [rels], full, full, full)
            kt = kernel_times(sess, _lib)
            _lib.call("capsmi_session_set_profiling", sess.handle, 0)
            sess.sync()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                graph.two_hop_count_distinct(sess, [rels], full, full, full)
            sess.sync()
            wall = (time.perf_counter() - t0) / args.steps * 1e3
            row[mode] = {"answer": answer, "kernels_ms": {k: round(v, 4) for k, v in kt.items()},
                         "wall_ms": round(wall, 3),
                         "after_pass1_ms": round(sum(v for k, v in kt.items() if k != "part_scatter1"), 4),
                         "ran": {"pool": sess.route_count("hop2_pool") - pool0,
                                 "cells": sess.route_count("hop2_cells") - cells0}}
            sess.set_config("CAPSMI_HOP2", None)
        doc["tables"].append(row)
        del rels
    sess.close()
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
