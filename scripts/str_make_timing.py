"""Timing of the functions that make a String (CAPSMI_X_TO_STRING, CAPSMI_X_CONCAT, k_strmake.hip), from the library's
own kernel timers (capsmi_session_kernel_time / _bytes): `str_index` (a String operand's code -> store index),
`str_make_lengths`, `str_make_starts` (the write pass's plan), `str_make` (the write pass), `str_store_merge` and its
plan `str_store_merge_starts`, and `str_make_gather`.  The distinct-tuple pass (the hash kernels) has no timer of its
own: it is the rest of the wall time beside the sink.  The sink -- the session's dictionary, in Python -- is timed on
the host around the callback, apart from the device's timers.

  toString(x) and s + x over n = 2^24 rows whose Long x draws from 2^12 and from 2^20 distinct values (s is one of 16
  strings, fixed by x, so the tuples are as many as the values).  The first run of a shape makes strings that are new
  to the store and merges them (reported apart, one sample); the 2 warm-up + 10 timed runs after it are the repeated
  query, in which the sink finds every string and nothing is merged.

Writes one JSON document (--out) and prints it.  Needs the GPU: there is no CPU path."""
import argparse
import ctypes
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cypher-for-apache-spark_amd"))

from explode_timing import stats  # noqa: E402
from list_expr_timing import HBM_BYTES_PER_S, wall_ms  # noqa: E402

TIMERS = ("str_index", "str_make_lengths", "str_make_starts", "str_make", "str_store_merge_starts", "str_store_merge",
          "str_make_gather")


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


def summary(rs):
    d = {}
    for name in TIMERS:
        if rs[0][name]["launches"] == 0:
            continue
        ms = stats([r[name]["ms"] for r in rs])
        d[name + "_ms"] = ms
        d[name + "_launches"] = rs[0][name]["launches"]
        if rs[0][name]["bytes"] > 0:
            d[name + "_declared_bytes"] = rs[0][name]["bytes"]
            d[name + "_gb_per_s"] = rs[0][name]["bytes"] / (ms["median"] * 1e-3) / 1e9
            d[name + "_of_roofline"] = d[name + "_gb_per_s"] * 1e9 / HBM_BYTES_PER_S
    d["timers_sum_ms"] = stats([sum(r[name]["ms"] for name in TIMERS) for r in rs])
    d["sink_ms"] = stats([r["sink_ms"] for r in rs])
    d["wall_ms"] = stats([r["wall_ms"] for r in rs])
    d["wall_minus_sink_ms"] = stats([r["wall_ms"] - r["sink_ms"] for r in rs])
    d["sink_strings"] = rs[0]["sink_strings"]
    return d


class TimedSink:
    """The session's own sink behind a wrapper that adds up the host time spent in it."""

    def __init__(self, s):
        from capsmi import _lib
        self.ms, self.strings = 0.0, 0

        def fn(ctx, n, offsets, data, out):
            t0 = time.perf_counter()
            rc = s._string_sink(ctx, n, offsets, data, out)
            self.ms += (time.perf_counter() - t0) * 1e3
            self.strings += n
            return rc

        self.cb = _lib.STRING_SINK_FN(fn)
        s.set_string_sink(self.cb)

    def take(self):
        ms, n = self.ms, self.strings
        self.ms, self.strings = 0.0, 0
        return ms, n


def runs(s, sink, a, log_values):
    from capsmi import ColumnData, expr
    from capsmi.expr import Col, Concat, ToString
    n, nv = 1 << a.log_rows, 1 << log_values
    rng = np.random.default_rng(25 + log_values)
    values = np.unique(rng.integers(-10 ** 12, 10 ** 12, nv + nv // 8))[:nv]
    assert len(values) == nv
    rng.shuffle(values)
    pick = rng.integers(0, nv, n)
    names = ["key%02d:" % k for k in range(16)]
    codes = np.array([s.dictionary.encode(x) for x in names], dtype=np.int64)
    t = s.table([ColumnData("x", expr.I64, values[pick]), ColumnData("s", expr.STR, codes[pick & 15])])
    digits = np.char.str_len(values.astype(str))
    doc = {}
    for name, e, out_bytes in (("toString", ToString(Col("x")), int(digits.sum())),
                               ("concat", Concat(Col("s"), Col("x")), int(digits.sum()) + 6 * nv)):
        first, rs = None, []
        for rep in range(1 + a.warmup + a.reps):
            w, out = wall_ms(s, lambda: (lambda o: (o, o.size))(t.withColumns((e, "r")))[0])
            r = read_timers(s)
            r["wall_ms"] = w
            r["sink_ms"], r["sink_strings"] = sink.take()
            if rep == 0:  # the strings are new: this run merges them into the store
                first = r
                c = out.column("r", 0, 4096)
                want = [(names[p & 15] if name == "concat" else "") + str(int(values[p])) for p in pick[:4096]]
                assert [s.dictionary.decode(int(v)) for v in c.values] == want, name
            elif rep > a.warmup:
                assert r["str_store_merge"]["launches"] == 0
                rs.append(r)
        doc[name] = {"output_bytes": out_bytes, "first_run": summary([first]), "repeated": summary(rs)}
    return {"rows": n, "distinct_values": nv, "ops": doc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log-values", default="12,20")
    ap.add_argument("--out", default=os.path.join("profiles", "r25_str_make.json"))
    a = ap.parse_args()
    from capsmi import Session, _lib
    s = Session(0)
    sink = TimedSink(s)
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    _lib.call("capsmi_session_set_profiling_names", s.handle, ",".join(TIMERS).encode())
    gc.collect()
    gc.disable()
    doc = {"reps": a.reps, "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S,
           "shapes": [runs(s, sink, a, int(lv)) for lv in a.log_values.split(",")]}
    s.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
