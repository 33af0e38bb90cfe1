"""Timing of the functions that read a String's characters (CAPSMI_X_STR_SIZE .. CAPSMI_X_TO_BOOLEAN, k_strconv.hip),
from the library's own kernel timers (capsmi_session_kernel_time / _bytes): `str_index` (code -> store index),
`str_conv_starts` (size only: byte lengths, scan, compaction), `str_conv` (the parse, or the tile pass of size) and
`str_conv_lookup` (the dictionary side's gather).  Declared bytes over the median time give each kernel's GB/s.

  parse: toInteger and toFloat over n = 2^24 rows that draw from 2^12 and from 2^20 distinct 8-byte numeric strings
         (eight digits, zero-padded), forced to the rows side (CAPSMI_STR_MATCH=rows) and to the dictionary side
         (=dict), alternating in one process.
  size:  size() on the rows side over 2^24 rows of 16 bytes each, one store entry per row, against the same number of
         bytes with one entry of 64 MiB among 16-byte ones.  The stores are registered with
         capsmi_session_set_strings itself (2^24 Python strings would cost more than the measurement).

Writes one JSON document (--out) and prints it.  Needs the GPU: there is no CPU path."""
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

TIMERS = ("str_index", "str_conv_starts", "str_conv", "str_conv_lookup")


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
    d["timers_sum_ms"] = stats([sum(r[name]["ms"] for name in TIMERS) for r in rs])
    d["wall_ms"] = stats([r["wall_ms"] for r in rs])
    return d


def with_column(s, t, op):
    """The table `t` with the column r = op(column 0), through the ABI (nothing re-registers the store)."""
    from capsmi import _lib, expr
    from capsmi.table import GpuTable, _EXPR_PTR
    prog = expr.to_ctypes([(expr.X_COL, 0, 0, 0), (op, 0, 0, 0)])
    cols = (_lib.ExprColumn * 1)()
    cols[0].name, cols[0].nnodes, cols[0].prog = b"r", 2, ctypes.cast(prog, _EXPR_PTR)
    h = ctypes.c_void_p()
    _lib.call("capsmi_with_columns", t._h, 1, cols, ctypes.byref(h))
    return GpuTable(s, h)


def set_store(s, codes, offsets, data):
    from capsmi import _lib
    _lib.call("capsmi_session_set_strings", s.handle, len(codes), codes.ctypes.data, offsets.ctypes.data, data.ctypes.data)


def parse_runs(s, a, log_strings):
    from capsmi import ColumnData, expr
    n, ns = 1 << a.log_rows, 1 << log_strings
    rng = np.random.default_rng(23)
    values = np.sort(rng.choice(10 ** 8, ns, replace=False))
    data = np.frombuffer("".join("%08d" % v for v in values).encode(), dtype=np.uint8).copy()
    codes = np.arange(ns, dtype=np.int64) * 3 + 7
    set_store(s, codes, np.arange(ns + 1, dtype=np.int64) * 8, data)
    pick = rng.integers(0, ns, n)
    t = s.table([ColumnData("s", expr.STR, codes[pick])])
    want = {expr.X_STR_TO_INTEGER: int(values[pick].sum()), expr.X_STR_TO_FLOAT: float(values[pick].astype(np.float64).sum())}
    doc = {}
    for name, op in (("toInteger", expr.X_STR_TO_INTEGER), ("toFloat", expr.X_STR_TO_FLOAT)):
        runs = {"rows": [], "dict": []}
        for rep in range(a.warmup + a.reps):
            for side in runs:  # alternating, in one process
                s.set_config("CAPSMI_STR_MATCH", side)
                w, out = wall_ms(s, lambda: (lambda o: (o, o.size))(with_column(s, t, op))[0])
                r = read_timers(s)
                r["wall_ms"] = w
                if rep == 0:
                    c = out.column("r")
                    assert c.valid is None or c.valid.all()
                    assert c.values.sum() == want[op], (name, side)
                if rep >= a.warmup:
                    runs[side].append(r)
        doc[name] = {side: summary(rs) for side, rs in runs.items()}
    return {"rows": n, "strings": ns, "string_bytes": int(len(data)), "ops": doc}


def size_runs(s, a):
    from capsmi import ColumnData, expr
    n = 1 << a.log_rows
    total = 16 * n
    rng = np.random.default_rng(24)
    data = rng.integers(ord("a"), ord("z") + 1, total, dtype=np.uint8)
    data[rng.integers(0, total, total // 64)] = 0xA9  # some continuation bytes, so the count is not the length
    lead = ((data & 0xC0) != 0x80).view(np.uint8)
    s.set_config("CAPSMI_STR_MATCH", "rows")
    doc = {"rows_uniform": n, "bytes": total}
    big = 64 << 20
    shapes = {"uniform": np.arange(n + 1, dtype=np.int64) * 16,
              "one_64MiB_string": np.concatenate([[0], big + np.arange(n - big // 16 + 1, dtype=np.int64) * 16])}
    runs = {k: [] for k in shapes}
    tables = {}
    for k, offsets in shapes.items():
        ne = len(offsets) - 1
        codes = np.arange(ne, dtype=np.int64)
        tables[k] = (codes, np.ascontiguousarray(offsets), np.add.reduceat(lead, offsets[:-1], dtype=np.int64),
                     s.table([ColumnData("s", expr.STR, codes)]))
    for rep in range(a.warmup + a.reps):
        for k, (codes, offsets, want, t) in tables.items():  # alternating; the store is replaced outside the timed part
            set_store(s, codes, offsets, data)
            w, out = wall_ms(s, lambda: (lambda o: (o, o.size))(with_column(s, t, expr.X_STR_SIZE))[0])
            r = read_timers(s)
            r["wall_ms"] = w
            if rep == 0:
                assert np.array_equal(out.column("r").values, want), k
            if rep >= a.warmup:
                runs[k].append(r)
    doc["shapes"] = {k: summary(rs) for k, rs in runs.items()}
    doc["rows_skewed"] = len(tables["one_64MiB_string"][0])
    doc["str_conv_ratio_skewed_over_uniform"] = (doc["shapes"]["one_64MiB_string"]["str_conv_ms"]["median"] /
                                                 doc["shapes"]["uniform"]["str_conv_ms"]["median"])
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--what", default="parse,size")
    ap.add_argument("--out", default=os.path.join("profiles", "r23_str_conv.json"))
    a = ap.parse_args()
    from capsmi import Session, _lib
    s = Session(0)
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    _lib.call("capsmi_session_set_profiling_names", s.handle, ",".join(TIMERS).encode())
    gc.collect()
    gc.disable()
    doc = {"reps": a.reps, "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S}
    if "parse" in a.what:
        doc["parse"] = [parse_runs(s, a, ls) for ls in (12, 20)]
    if "size" in a.what:
        doc["size"] = size_runs(s, a)
    s.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
