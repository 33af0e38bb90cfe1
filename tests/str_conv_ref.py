"""A pure-Python restatement of size(), toInteger(), toFloat() and toBoolean() of a String, as include/capsmi.h
states them for CAPSMI_X_STR_SIZE .. CAPSMI_X_TO_BOOLEAN (the Spark 2.2.1 calls SparkSQLExprMapper.scala:124-127,
:231, :229 and :235 make: UTF8String.numChars, UTF8String.toInt, Double.parseDouble, StringUtils.isTrueString /
isFalseString).  Every function takes the string's bytes (or a str, encoded as UTF-8) and returns None for NULL.

toFloat checks the grammar itself with regular expressions and leaves the value to ``float()`` (decimals) and
``float.fromhex`` (hex floats), which are correctly rounded conversions when ``sys.float_repr_style`` is "short"."""
import re
import struct
import sys

assert sys.float_repr_style == "short", "float() is the correctly rounded conversion only with the short repr"

NAN_BITS = 0x7FF8000000000000  # Double.NaN


def _bytes(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


def bits_of(d: float) -> int:
    """The double's bit pattern as a signed 64-bit word (the column word of a Double)."""
    return struct.unpack("<q", struct.pack("<d", d))[0]


def size(s):
    if s is None:
        return None
    return sum(1 for b in _bytes(s) if b & 0xC0 != 0x80)


_INT = re.compile(rb"([+-]?)([0-9]*)(\.[0-9]*)?", re.S)


def to_integer(s):
    if s is None:
        return None
    b = _bytes(s)
    m = _INT.fullmatch(b)
    if not m or b in (b"", b"+", b"-"):
        return None
    digits = m.group(2).lstrip(b"0")
    if len(digits) > 10:  # beyond 32 bits at any number of digits
        return None
    v = int(digits or b"0")
    if m.group(1) == b"-":
        v = -v
    return v if -(1 << 31) <= v < (1 << 31) else None


_DEC = re.compile(rb"([+-]?)((?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?)[fFdD]?", re.S)
_HEX = re.compile(rb"([+-]?)0[xX]((?:[0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)[pP][+-]?[0-9]+)[fFdD]?", re.S)
_WORD = re.compile(rb"([+-]?)(NaN|Infinity)", re.S)


def to_float(s):
    """The double, or None.  NaN is Double.NaN whatever sign the text carries (compare with ``to_float_bits``)."""
    if s is None:
        return None
    b = _bytes(s)
    lo, hi = 0, len(b)
    while lo < hi and b[lo] <= 0x20:
        lo += 1
    while hi > lo and b[hi - 1] <= 0x20:
        hi -= 1
    b = b[lo:hi]
    m = _WORD.fullmatch(b)
    if m:
        if m.group(2) == b"NaN":
            return float("nan")
        return float("-inf") if m.group(1) == b"-" else float("inf")
    neg = b[:1] == b"-"
    m = _HEX.fullmatch(b)
    if m:
        try:
            v = float.fromhex("0x" + m.group(2).decode("ascii"))
        except OverflowError:
            v = float("inf")
        return -v if neg else v
    m = _DEC.fullmatch(b)
    if m:
        v = float(m.group(2).decode("ascii"))  # overflow gives inf, underflow 0.0
        return -v if neg else v
    return None


def to_float_bits(s):
    v = to_float(s)
    if v is None:
        return None
    return NAN_BITS if v != v else bits_of(v)


_TRUE, _FALSE = (b"t", b"true", b"y", b"yes", b"1"), (b"f", b"false", b"n", b"no", b"0")


def to_boolean(s):
    if s is None or isinstance(s, bool):
        return s
    b = bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in _bytes(s))
    return True if b in _TRUE else (False if b in _FALSE else None)


FUNCS = {"str_size": size, "str_tointeger": to_integer, "str_tofloat": to_float, "toboolean": to_boolean}


def word_of(op: str, s):
    """(value word, validity) as the device writes them: the Double's bits for str_tofloat, 0 / 1 for toboolean."""
    if op == "str_tofloat":
        v = to_float_bits(s)
        if v is not None and v >= 1 << 63:
            v -= 1 << 64
    else:
        v = FUNCS[op](s)
    return (0, 0) if v is None else (int(v), 1)
