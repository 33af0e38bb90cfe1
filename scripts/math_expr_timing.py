"""Expression-interpreter timing for the numeric opcodes: the `expr_eval` kernel timer (capsmi_session_kernel_time)
of withColumns over n = 2^24 rows for
  - `x * y + 1.0`, which holds none of the new opcodes and so runs the plain instantiation of k_eval, on this build
    and, with --parent, on a build of the parent commit (`make` in a checkout of it, the library copied aside),
    alternating in one process: the same code is expected, the margin is the parent's own min - max;
  - `sqrt(x)`, `log(x)` and `x / y`, which run the math instantiation (this build only).
x and y are Doubles without nulls (seeded, positive).  Bytes per row: 8 read per operand, 8 + 1 written (value and
validity); that over the median time, against the 8 TB/s of HBM, is the share of the roofline.  Writes one JSON
document (--out) and prints it.  Needs the GPU: there is no CPU path.

Two builds in one process: each is its own ctypes library with its own session and tables; the binding's current
library is switched between them, and every table made under one is dropped before the switch."""
import argparse
import ctypes
import gc
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cypher-for-apache-spark_amd"))

from explode_timing import stats  # noqa: E402
from list_expr_timing import HBM_BYTES_PER_S, wall_ms  # noqa: E402

TIMER = "expr_eval"


def open_library(path):
    from capsmi import _lib
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib._SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def use(lib):
    from capsmi import _lib
    _lib._lib = lib
    _lib._FN.clear()


def read_timer(s):
    from capsmi import _lib
    cnt, ms = ctypes.c_int64(), ctypes.c_double()
    _lib.call("capsmi_session_kernel_time", s.handle, TIMER.encode(), ctypes.byref(cnt), ctypes.byref(ms))
    return cnt.value, ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent", default=None, help="libcapsmi.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join("profiles", "r16_math_expr.json"))
    a = ap.parse_args()
    from capsmi import ColumnData, Session, _lib
    from capsmi.expr import F64, BinOp, Col, Lit, Log, Sqrt
    n = 1 << a.log_rows
    rng = np.random.default_rng(15)
    x = rng.uniform(0.5, 1000.0, n)
    y = rng.uniform(0.5, 1000.0, n)
    exprs = {"mul_add": (BinOp("+", BinOp("*", Col("x"), Col("y")), Lit(1.0)), 2, x * y + 1.0),
             "sqrt": (Sqrt(Col("x")), 1, np.sqrt(x)),
             "log": (Log(Col("x")), 1, np.log(x)),
             "div": (BinOp("/", Col("x"), Col("y")), 2, x / y)}
    builds = {"this": _lib.load()}
    if a.parent:
        builds["parent"] = open_library(a.parent)
    sessions, tables = {}, {}
    for b, lib in builds.items():
        use(lib)
        s = sessions[b] = Session(0)
        tables[b] = s.table([ColumnData("x", F64, x), ColumnData("y", F64, y)])
        _lib.call("capsmi_session_set_profiling", s.handle, 1)
        _lib.call("capsmi_session_set_profiling_names", s.handle, TIMER.encode())
    runs = {(b, k): [] for b in builds for k in exprs if b == "this" or k == "mul_add"}
    checked = set()
    gc.collect()
    gc.disable()
    for rep in range(a.warmup + a.reps):
        for (b, k) in runs:  # alternating, in one process
            use(builds[b])
            s, (e, _, want) = sessions[b], exprs[k]
            read_timer(s)  # reset
            out = tables[b].withColumns((e, "r"))
            w, _ = wall_ms(s, lambda: out.size)
            launches, ms = read_timer(s)
            assert launches == 1, (b, k, launches)
            if (b, k) not in checked:  # the timed work computes what numpy computes (log: to 2 ULP)
                got = out.column("r").values
                assert np.allclose(got, want, rtol=1e-15, atol=0.0) if k == "log" else np.array_equal(got, want), (b, k)
                checked.add((b, k))
            del out  # before the next build's turn
            if rep >= a.warmup:
                runs[(b, k)].append({"ms": ms, "wall_ms": w})
    doc = {"rows": n, "reps": a.reps, "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S, "timer": TIMER,
           "parent_library": a.parent and os.path.basename(a.parent), "builds": {b: {} for b in builds}}
    for (b, k), rs in runs.items():
        ms = stats([r["ms"] for r in rs])
        nbytes = n * (8 * exprs[k][1] + 9)
        doc["builds"][b][k] = {"expr_eval_ms": ms, "wall_ms": stats([r["wall_ms"] for r in rs]), "bytes": nbytes,
                               "gb_per_s": nbytes / (ms["median"] * 1e-3) / 1e9,
                               "share_of_hbm_roofline": nbytes / (ms["median"] * 1e-3) / HBM_BYTES_PER_S}
    for b in builds:  # each session and its table under its own library
        use(builds[b])
        tables.pop(b)
        sessions[b].close()
    use(builds["this"])
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
