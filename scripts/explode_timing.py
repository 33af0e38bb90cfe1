"""UNWIND timing: the column explode at n = 2^22 rows, m = 2^26 I64 elements, two payload columns, for
  (a) uniform: every list 16 elements;
  (b) skewed:  one list holding m / 2, half the rows empty, the rest spread geometrically,
alternating in one process, from the library's own kernel timers (capsmi_session_kernel_time / _bytes):
`explode` (tile-head search + expansion kernel; its declared algorithmic bytes over the 8 TB/s HBM peak give
the roofline share), `explode_starts` (lengths, scan, compaction) and `explode_gather` (the payload columns,
apart).  The skewed case is judged against the uniform case of the same run and that run's own spread.
Writes one JSON document (--out) and prints it.  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cypher-for-apache-spark_amd"))

HBM_BYTES_PER_S = 8e12
TIMERS = ("explode", "explode_starts", "explode_gather")


def lengths(case, n, m, rng):
    if case == "uniform":
        return np.full(n, m // n, dtype=np.int64)
    lens = np.zeros(n, dtype=np.int64)
    rows = rng.permutation(n)[: n // 2]          # the other half stays empty
    rest = rng.geometric(1.0 / (m / 2 / (len(rows) - 1)), len(rows) - 1).astype(np.int64)
    diff = m // 2 - int(rest.sum())              # make the spread part add up to m / 2 exactly
    while diff != 0:
        k = rng.integers(0, len(rest), min(abs(diff), len(rest)))
        step = np.sign(diff)
        ok = rest[k] + step >= 1
        np.add.at(rest, k[ok], step)
        diff = m // 2 - int(rest.sum())
    lens[rows[0]] = m // 2
    lens[rows[1:]] = rest
    return lens


def table(s, lens, rng):
    from capsmi import ColumnData
    from capsmi.expr import I64
    n = len(lens)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    vals = rng.integers(-(1 << 40), 1 << 40, int(offs[-1]), dtype=np.int64)
    t = s.table([ColumnData("a", I64, np.arange(n, dtype=np.int64)), ColumnData("b", I64, rng.integers(0, 1 << 30, n))])
    return t.add_list_column_csr("xs", I64, offs, vals)


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


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=22)
    ap.add_argument("--log-elements", type=int, default=26)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r08_explode.json"))
    a = ap.parse_args()
    from capsmi import Session, _lib
    n, m = 1 << a.log_rows, 1 << a.log_elements
    rng = np.random.default_rng(8)
    s = Session(0)
    tables = {c: table(s, lengths(c, n, m, rng), rng) for c in ("uniform", "skewed")}
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    _lib.call("capsmi_session_set_profiling_names", s.handle, ",".join(TIMERS).encode())
    runs = {c: [] for c in tables}
    for rep in range(a.warmup + a.reps):
        for c, t in tables.items():  # alternating, in one process
            out = t.explode("xs", "item")
            assert out.size == m
            del out
            r = read_timers(s)
            if rep >= a.warmup:
                runs[c].append(r)
    doc = {"rows": n, "elements": m, "element_type": "I64", "payload_columns": 2, "reps": a.reps, "warmup": a.warmup,
           "hbm_peak_bytes_per_s": HBM_BYTES_PER_S, "cases": {}}
    for c, rs in runs.items():
        ex = stats([r["explode"]["ms"] for r in rs])
        nbytes = rs[0]["explode"]["bytes"]
        doc["cases"][c] = {
            "explode_ms": ex,
            "explode_algorithmic_bytes": nbytes,
            "explode_roofline_fraction": nbytes / (ex["median"] * 1e-3) / HBM_BYTES_PER_S,
            "explode_starts_ms": stats([r["explode_starts"]["ms"] for r in rs]),
            "explode_gather_ms": stats([r["explode_gather"]["ms"] for r in rs]),
        }
    u, k = doc["cases"]["uniform"]["explode_ms"], doc["cases"]["skewed"]["explode_ms"]
    doc["skewed_over_uniform_median"] = k["median"] / u["median"]
    doc["uniform_spread_max_over_min"] = u["max"] / u["min"]
    doc["skewed_within_uniform_spread"] = bool(u["min"] <= k["median"] <= u["max"])
    s.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
