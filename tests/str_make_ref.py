"""The rules of toString() and string concatenation (include/capsmi.h, CAPSMI_X_TO_STRING and CAPSMI_X_CONCAT) in pure
Python: Java's Long.toString is Python's str of an int, a Boolean gives ``true`` / ``false``, a String stays, and a
concatenation is the bytes of the first operand followed by those of the second, a Long formatted first.  None is NULL
and makes the result NULL.  A Double raises NotImplementedError: the device path does not restate Double.toString."""

LONG_MIN, LONG_MAX = -(1 << 63), (1 << 63) - 1


def to_string(x):
    if x is None:
        return None
    if isinstance(x, bool):
        return "true" if x else "false"
    if isinstance(x, int):
        assert LONG_MIN <= x <= LONG_MAX
        return str(x)
    if isinstance(x, float):
        raise NotImplementedError("Double.toString")
    if isinstance(x, str):
        return x
    raise TypeError(type(x))


def concat(a, b):
    for x in (a, b):
        if isinstance(x, float):
            raise NotImplementedError("Double.toString")
        if isinstance(x, bool):
            raise ValueError("a Boolean operand of a concatenation")
    if a is None or b is None:
        return None
    if isinstance(a, int) and isinstance(b, int):
        raise ValueError("Long + Long is an addition")
    return to_string(a) + to_string(b)


def edge_longs():
    """0, +-1, 9, 10, 99, 100, +-10^k and 10^k - 1 for k = 1..18, Long.MAX and Long.MIN."""
    vals = [0, 1, -1, 9, 10, 99, 100]
    for k in range(1, 19):
        vals += [10 ** k, -(10 ** k), 10 ** k - 1]
    vals += [LONG_MAX, LONG_MIN]
    out = []
    for v in vals:
        if v not in out:
            out.append(v)
    return out


FUNCS = {"tostring": to_string, "concat": concat}
