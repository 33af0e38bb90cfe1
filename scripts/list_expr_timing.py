"""List-expression timing: x IN list-column and range() at n = 2^22 rows, M = 2^26 I64 elements, for
  (a) uniform: every list 16 elements;
  (b) skewed:  one list holding M / 2, half the rows empty, the rest spread geometrically,
alternating in one process, from the library's own kernel timers (capsmi_session_kernel_time / _bytes):
`list_contains` (tile-head search + membership kernel; its declared algorithmic bytes, 8 B x (3 n + M), over the
8 TB/s HBM peak give the roofline share), `list_contains_starts` (lengths, scan, compaction), and the same pair
for `list_range`.  The skewed case is judged against the uniform case of the same run and that run's own spread.
For comparison the wall time of the whole membership column (lengths to finish, synchronised) stands next to the
wall time of the only route the library had before for the same answer, on the same data:
explode -> filter(item = p) -> distinct on the row id.  Probes are drawn so that about half the rows with a
non-empty list hold their probe.  Writes one JSON document (--out) and prints it.  Needs the GPU: there is no
CPU path."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cypher-for-apache-spark_amd"))

from explode_timing import lengths, stats  # noqa: E402  (the two length distributions of the UNWIND timing)

HBM_BYTES_PER_S = 8e12
TIMERS = ("list_contains", "list_contains_starts", "list_range", "list_range_starts")


def table(s, lens, rng):
    from capsmi import ColumnData
    from capsmi.expr import I64
    n = len(lens)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    vals = rng.integers(0, 1 << 40, int(offs[-1]), dtype=np.int64)
    # the probe: an element of the row's own list for every other row, else a value no list holds
    probe = np.full(n, -1, dtype=np.int64)
    pick = (np.arange(n) % 2 == 0) & (lens > 0)
    probe[pick] = vals[offs[:-1][pick] + lens[pick] // 2]
    t = s.table([ColumnData("a", I64, np.arange(n, dtype=np.int64)), ColumnData("p", I64, probe),
                 ColumnData("last", I64, lens - 1)])  # range(0, last) has the row's list length
    return t.add_list_column_csr("xs", I64, offs, vals), int(pick.sum())


def read_timers(s):
    from capsmi import _lib
    out = {}
    for name in TIMERS:
        nb = ctypes.c_double()
        _lib.call("capsmi_session_kernel_bytes", s.handle, name.encode(), ctypes.byref(nb))
        k, ms = ctypes.c_int64(), ctypes.c_double()
        _lib.call("capsmi_session_kernel_time", s.handle, name.encode(), ctypes.byref(k), ctypes.byref(ms))
        out[name] = {"launches": k.value, "ms": ms.value, "bytes": nb.value}
    return out


def wall_ms(s, f):
    s.sync()
    t0 = time.perf_counter()
    r = f()
    s.sync()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=22)
    ap.add_argument("--log-elements", type=int, default=26)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r09_list_expr.json"))
    a = ap.parse_args()
    from capsmi import Session, _lib
    from capsmi.expr import BinOp, Col, InList, Lit
    n, m = 1 << a.log_rows, 1 << a.log_elements
    rng = np.random.default_rng(9)
    s = Session(0)
    tables, present = {}, {}
    for c in ("uniform", "skewed"):
        tables[c], present[c] = table(s, lengths(c, n, m, rng), rng)
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    _lib.call("capsmi_session_set_profiling_names", s.handle, ",".join(TIMERS).encode())
    runs = {c: [] for c in tables}
    for rep in range(a.warmup + a.reps):
        for c, t in tables.items():  # alternating, in one process
            w_in, hits = wall_ms(s, lambda: t.filter(InList(Col("p"), Col("xs"))).size)
            assert hits == present[c], (hits, present[c])
            w_old, old_hits = wall_ms(s, lambda: t.explode("xs", "item").filter(BinOp("=", Col("item"), Col("p")))
                                      .distinct("a").size)
            assert old_hits == hits
            w_rg, rg = wall_ms(s, lambda: t.withRangeColumn(Lit(0), Col("last"), None, "rg").select("rg"))
            w_rg2, _ = wall_ms(s, lambda: rg.size)
            del rg
            r = read_timers(s)
            r["wall"] = {"in_list_filter_ms": w_in, "explode_filter_distinct_ms": w_old, "range_column_ms": w_rg + w_rg2}
            if rep >= a.warmup:
                runs[c].append(r)
    doc = {"rows": n, "elements": m, "element_type": "I64", "reps": a.reps, "warmup": a.warmup,
           "hbm_peak_bytes_per_s": HBM_BYTES_PER_S, "rows_holding_their_probe": present, "cases": {}}
    for c, rs in runs.items():
        d = {}
        for k in ("list_contains", "list_range"):
            ms = stats([r[k]["ms"] for r in rs])
            nbytes = rs[0][k]["bytes"]
            d[k + "_ms"] = ms
            d[k + "_algorithmic_bytes"] = nbytes
            d[k + "_roofline_fraction"] = nbytes / (ms["median"] * 1e-3) / HBM_BYTES_PER_S
            d[k + "_starts_ms"] = stats([r[k + "_starts"]["ms"] for r in rs])
        for k in ("in_list_filter_ms", "explode_filter_distinct_ms", "range_column_ms"):
            d["wall_" + k] = stats([r["wall"][k] for r in rs])
        d["explode_route_over_in_list_wall"] = d["wall_explode_filter_distinct_ms"]["median"] / d["wall_in_list_filter_ms"]["median"]
        doc["cases"][c] = d
    for k in ("list_contains", "list_range"):
        u, sk = doc["cases"]["uniform"][k + "_ms"], doc["cases"]["skewed"][k + "_ms"]
        doc[k + "_skewed_over_uniform_median"] = sk["median"] / u["median"]
        doc[k + "_uniform_spread_max_over_min"] = u["max"] / u["min"]
        doc[k + "_skewed_within_uniform_spread"] = bool(u["min"] <= sk["median"] <= u["max"])
    s.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
