"""CONTAINS timing: Contains(column, 3-byte literal) at n = 2^24 rows over a string store of 2^20 distinct strings
(8 to 24 letters of an 11-letter alphabet, mean 16 bytes, seeded; about 1 % of the strings hold the literal), forced
to the row side (CAPSMI_STR_MATCH=rows: one candidate slot per start position of every row) and to the dictionary side
(=dict: the slots of the store's entries, then one lookup per row), alternating in one process, from the library's own
kernel timers (capsmi_session_kernel_time / _bytes): `str_index` (code -> store index), `str_match_starts` (slot
counts, scan, compaction), `str_match` (tile heads + the compare) and `str_match_lookup` / `str_match_finish` (the
three-valued result per row).  Declared bytes over the median time give each kernel's GB/s.  Writes one JSON document
(--out) and prints it.  Needs the GPU: there is no CPU path."""
import argparse
import gc
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cypher-for-apache-spark_amd"))

from explode_timing import stats  # noqa: E402
from list_expr_timing import HBM_BYTES_PER_S, wall_ms  # noqa: E402

TIMERS = ("str_index", "str_match_starts", "str_match", "str_match_lookup", "str_match_finish")
ALPHABET = "abcdefghijk"
PATTERN = "abc"


def strings(count, rng):
    """`count` distinct strings of 8 to 24 letters."""
    out = set()
    while len(out) < count:
        k = count - len(out) + 1024
        lens = rng.integers(8, 25, k)
        letters = rng.integers(0, len(ALPHABET), (k, 24)).astype(np.uint8) + ord(ALPHABET[0])
        for row, ln in zip(letters, lens):
            out.add(row[:ln].tobytes().decode())
            if len(out) == count:
                break
    return sorted(out)


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
    ap.add_argument("--log-strings", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "r13_str_match.json"))
    a = ap.parse_args()
    from capsmi import ColumnData, Session, _lib
    from capsmi.expr import STR, Col, Contains, Lit
    n, ns = 1 << a.log_rows, 1 << a.log_strings
    rng = np.random.default_rng(13)
    pool = strings(ns, rng)
    s = Session(0)
    s.dictionary.extend(pool + [PATTERN])
    codes = np.array([s.dictionary.encode(x) for x in pool], dtype=np.int64)
    pick = rng.integers(0, ns, n)
    t = s.table([ColumnData("s", STR, codes[pick])])
    holds = np.array([PATTERN in x for x in pool])
    want = int(holds[pick].sum())
    _lib.call("capsmi_session_set_profiling", s.handle, 1)
    _lib.call("capsmi_session_set_profiling_names", s.handle, ",".join(TIMERS).encode())
    runs = {"rows": [], "dict": []}
    gc.collect()
    gc.disable()  # a full collection over the 2^20 strings held here costs tens of milliseconds of wall time
    for rep in range(a.warmup + a.reps):
        for side in runs:  # alternating, in one process
            s.set_config("CAPSMI_STR_MATCH", side)
            w, got = wall_ms(s, lambda: t.filter(Contains(Col("s"), Lit(PATTERN))).size)
            assert got == want, (got, want)
            r = read_timers(s)
            r["wall_ms"] = w
            if rep >= a.warmup:
                runs[side].append(r)
    doc = {"rows": n, "strings": len(s.dictionary), "string_bytes": int(sum(len(x) for x in pool)) + len(PATTERN),
           "pattern": PATTERN, "matching_rows": want, "matching_strings": int(holds.sum()), "reps": a.reps,
           "warmup": a.warmup, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S, "sides": {}}
    for side, rs in runs.items():
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
        doc["sides"][side] = d
    s.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
