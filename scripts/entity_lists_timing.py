"""labels() timing: capsmi_with_mask_list_column (CAPSMI_MASK_TRUE) at n = 2^24 rows over K = 16 nullable Boolean
flag columns, M about 2^27 String elements, for
  (a) uniform: every flag TRUE with probability 1/2;
  (b) skewed:  half the rows have no TRUE flag, the rest have all 16,
alternating in one process, from the library's own kernel timers (capsmi_session_kernel_time / _bytes):
`mask_list_len` (one mask word, length and flag per row; declared 9 B per row and nullable column read, 17 B per
row written), `mask_list_starts` (scan of the lengths and compaction of the non-empty rows) and `mask_list`
(tile-head search + fill; declared 8 B x (2 n + M)).  Declared bytes over the 8 TB/s HBM peak give each kernel's
roofline share.  The skewed case is judged against the uniform case of the same run and that run's own spread.
One cell in eight that is not TRUE is a NULL over a random word instead of a FALSE.  Writes one JSON document
(--out) and prints it.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cypher-for-apache-spark_amd"))

from explode_timing import stats  # noqa: E402
from list_expr_timing import HBM_BYTES_PER_S, wall_ms  # noqa: E402

TIMERS = ("mask_list_len", "mask_list_starts", "mask_list")


def table(s, case, n, k, rng):
    """(table of k nullable flag columns f00 .., the number of TRUE non-null flags)"""
    from capsmi import ColumnData
    from capsmi.expr import BOOL
    full = rng.permutation(n) < n // 2 if case == "skewed" else None
    cols, m = [], 0
    for i in range(k):
        true = full if case == "skewed" else rng.random(n) < 0.5
        null = ~true & (rng.integers(0, 8, n) == 0)
        word = np.where(null, rng.integers(0, 2, n), true).astype(np.int64)
        cols.append(ColumnData(f"f{i:02d}", BOOL, word, ~null))
        m += int(true.sum())
    return s.table(cols), m


def read_timers(s):
    import ctypes
    from capsmi import _lib
    out = {}
    for name in TIMERS:
        nb = ctypes.c_double()
        _lib.call("capsmi_session_kernel_bytes", s.handle, name.encode(), ctypes.byref(nb))
        cnt, ms = ctypes.c_int64(), ctypes.c_double()
        _lib.call("capsmi_session_kernel_time", s.handle, name.encode(), ctypes.byref(cnt), ctypes.byref(ms))
        out[name] = {"launches": cnt.value, "ms": ms.value, "bytes": nb.value}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", type=int, default=24)
    ap.add_argument("--columns", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r10_entity_lists.json"))
    a = ap.parse_args()
    from capsmi import Session, _lib
    from capsmi.expr import MASK_TRUE
    n, k = 1 << a.log_rows, a.columns
    rng = np.random.default_rng(10)
    s = Session(0)
    cols, names = [f"f{i:02d}" for i in range(k)], [f"L{i:02d}" for i in range(k)]
    tables, elements = {}, {}
    for c in ("uniform", "skewed"):
        tables[c], elements[c] = table(s, c, n, k, rng)
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    _lib.call("capsmi_session_set_profiling_names", s.handle, ",".join(TIMERS).encode())
    runs = {c: [] for c in tables}
    for rep in range(a.warmup + a.reps):
        for c, t in tables.items():  # alternating, in one process
            w, out = wall_ms(s, lambda: t.withMaskListColumn(MASK_TRUE, cols, names, "l").select("l"))
            w2, rows = wall_ms(s, lambda: out.size)
            assert rows == n
            del out
            r = read_timers(s)
            r["wall_ms"] = w + w2
            if rep >= a.warmup:
                runs[c].append(r)
    doc = {"rows": n, "columns": k, "mode": "CAPSMI_MASK_TRUE", "flags": "nullable BOOL", "elements": elements,
           "reps": a.reps, "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S, "cases": {}}
    for c, rs in runs.items():
        d = {}
        for name in TIMERS:
            ms = stats([r[name]["ms"] for r in rs])
            d[name + "_ms"] = ms
            d[name + "_launches"] = rs[0][name]["launches"]
            if rs[0][name]["bytes"] > 0:
                d[name + "_declared_bytes"] = rs[0][name]["bytes"]
                d[name + "_roofline_fraction"] = rs[0][name]["bytes"] / (ms["median"] * 1e-3) / HBM_BYTES_PER_S
        d["wall_ms"] = stats([r["wall_ms"] for r in rs])
        doc["cases"][c] = d
    u, sk = doc["cases"]["uniform"]["mask_list_ms"], doc["cases"]["skewed"]["mask_list_ms"]
    doc["mask_list_skewed_over_uniform_median"] = sk["median"] / u["median"]
    doc["mask_list_uniform_spread_max_over_min"] = u["max"] / u["min"]
    doc["mask_list_skewed_within_uniform_spread"] = bool(u["min"] <= sk["median"] <= u["max"])
    s.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
