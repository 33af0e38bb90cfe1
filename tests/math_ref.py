"""Pure-Python restatement of the numeric expression opcodes (include/capsmi.h, CAPSMI_X_DIV .. CAPSMI_X_TO_INTEGER):
what Spark 2.2.1 does with the Column calls of SparkSQLExprMapper.scala:186, :229-231 and :249-260, stated from
knowledge of Spark's source.  A Long is a Python int, a Double a Python float, NULL is None; a bool or a str is no
number and gives NULL, as on the device.  Every function returns an int for a Long result and a float for a Double
result, so ``same_value`` can compare type, bits (the sign of zero) and validity."""
import decimal
import math
import struct

LONG_MAX, LONG_MIN = (1 << 63) - 1, -(1 << 63)
INT_MAX, INT_MIN = (1 << 31) - 1, -(1 << 31)
LN10 = 2.302585092994046  # the double log(10.0)

OPS = ("sqrt", "log", "log10", "exp", "abs", "ceil", "floor", "round", "sign", "tofloat", "tointeger")


def _num(v):
    return v is not None and not isinstance(v, (bool, str)) and isinstance(v, (int, float))


def sat_i64(d: float) -> int:
    """Java's (long) d."""
    if d != d:
        return 0
    if d >= 2.0 ** 63:
        return LONG_MAX
    if d <= -(2.0 ** 63):
        return LONG_MIN
    return int(d)  # toward zero


def wrap_i64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def div(a, b):
    if not _num(a) or not _num(b):
        return None
    p, q = float(a), float(b)  # Spark's Division works on doubles; int -> float rounds to nearest
    if q == 0.0:
        return None
    d = p / q  # float division raises for a zero divisor only: inf / inf is NaN, an overflow is inf
    return sat_i64(d) if isinstance(a, int) and isinstance(b, int) else d


def sqrt(x):
    if not _num(x):
        return None
    x = float(x)
    if x != x or x < 0.0:
        return math.nan
    return math.sqrt(x)  # -0.0 -> -0.0, inf -> inf


def log(x):
    if not _num(x):
        return None
    x = float(x)
    if x <= 0.0:
        return None
    return math.log(x)  # NaN -> NaN, inf -> inf


def log10(x):
    v = log(x)
    return None if v is None else v / LN10


def exp(x):
    if not _num(x):
        return None
    try:
        return math.exp(float(x))
    except OverflowError:
        return math.inf


def abs_(x):
    if not _num(x):
        return None
    if isinstance(x, int):
        return wrap_i64(-x) if x < 0 else x
    return math.copysign(x, 1.0)


def _via_long(x, f):
    if not _num(x):
        return None
    if isinstance(x, int):
        return float(x)
    if x != x or math.isinf(x):
        return float(sat_i64(x))
    return float(max(LONG_MIN, min(LONG_MAX, f(x))))  # math.ceil / math.floor are exact integers


def ceil(x):
    return _via_long(x, math.ceil)


def floor(x):
    return _via_long(x, math.floor)


def round_(x):
    if not _num(x):
        return None
    if isinstance(x, int) or x != x or math.isinf(x) or abs(x) >= 2.0 ** 52:
        return float(x)
    r = float(decimal.Decimal(x).quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_UP))
    return r + 0.0  # BigDecimal has no signed zero


def sign(x):
    if not _num(x):
        return None
    x = float(x)
    return (x > 0.0) - (x < 0.0)


def tofloat(x):
    return float(x) if _num(x) else None


def tointeger(x):
    if not _num(x):
        return None
    if isinstance(x, int):
        v = x & 0xFFFFFFFF
        return v - (1 << 32) if v >= 1 << 31 else v
    if x != x:
        return 0
    if x >= INT_MAX:
        return INT_MAX
    if x <= INT_MIN:
        return INT_MIN
    return int(x)


FUNCS = {"sqrt": sqrt, "log": log, "log10": log10, "exp": exp, "abs": abs_, "ceil": ceil, "floor": floor,
         "round": round_, "sign": sign, "tofloat": tofloat, "tointeger": tointeger}


def bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def same_value(got, want) -> bool:
    """Type, validity and bits: +0.0 is not -0.0; every NaN is one NaN."""
    if got is None or want is None:
        return got is None and want is None
    if type(got) is not type(want):
        return False
    if isinstance(want, float):
        return (got != got and want != want) or bits(got) == bits(want)
    return got == want


def eval_spec(spec, row):
    """A planner DSL expression over ``row`` (variable -> {"props": ..})."""
    op = spec[0]
    if op == "lit":
        return spec[1]
    if op == "prop":
        return row[spec[1]]["props"].get(spec[2])
    if op == "e":
        return math.e
    if op == "/":
        return div(eval_spec(spec[1], row), eval_spec(spec[2], row))
    if op in FUNCS:
        return FUNCS[op](eval_spec(spec[1], row))
    raise NotImplementedError(op)
