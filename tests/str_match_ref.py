"""Shared by test_string_predicates_cpu.py and test_gpu_string_predicates.py: a pure-Python three-valued restatement
of STARTS WITH / ENDS WITH / CONTAINS over the UTF-8 bytes of the operands (Spark's UTF8String.startsWith / endsWith /
contains compare bytes), and T, the tile of candidate slots that CONTAINS runs over."""
T = 2048  # kExplodeTile (capsmi_impl.h)

OPS = ("starts_with", "ends_with", "contains")


def as_bytes(v):
    """The bytes StringDictionary.arrays() stores for v: UTF-8, a surrogate escape (PEP 383) as the byte it stands for."""
    return v.encode("utf-8", "surrogateescape") if isinstance(v, str) else v


def ref_match(op, s, p):
    """None when either operand is None; else whether the bytes of p begin / end / occur in the bytes of s.  The
    empty pattern matches every string; a pattern longer than the string never matches."""
    if s is None or p is None:
        return None
    s, p = as_bytes(s), as_bytes(p)
    if len(p) > len(s):
        return False
    if op == "starts_with":
        return s[:len(p)] == p
    if op == "ends_with":
        return s[len(s) - len(p):] == p
    if op == "contains":
        return any(s[i:i + len(p)] == p for i in range(len(s) - len(p) + 1))
    raise ValueError(op)


def slots(s, p):
    """Candidate slots of one row of CONTAINS: start positions at which the pattern still fits."""
    if s is None or p is None or len(as_bytes(p)) == 0:
        return 0
    return max(0, len(as_bytes(s)) - len(as_bytes(p)) + 1)
