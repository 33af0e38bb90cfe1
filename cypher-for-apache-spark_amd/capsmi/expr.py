"""Expression trees handed to ``Table.filter`` / ``Table.withColumns``.

The analogue of okapi's ``Expr`` hierarchy (okapi-ir/src/main/scala/org/opencypher/okapi/ir/api/expr/Expr.scala)
restricted to what SparkSQLExprMapper maps for the pattern-matching path
(spark-cypher/src/main/scala/org/opencypher/spark/impl/SparkSQLExprMapper.scala:81-312):
column references (a Var / Property / HasLabel / HasType resolves to a physical column of the
RecordHeader, :97-105), literals and parameters (:86-92, :111-117), Equals (:120), Not (:121),
IsNull / IsNotNull (:122-123), Ands / Ors (:132-136), In (:138-145), < <= > >= (:147-150),
Add / Subtract / Multiply, and the id-tag vocabulary BitwiseAnd / BitwiseOr / ShiftLeft /
ShiftRightUnsigned (:264-274), CaseExpr (:283-298), and Explode of a list column, ListLit or list
parameter (:237-241), which ``GpuTable.withColumns`` runs as the UNWIND operator.

List expressions: Size (:124-130; NULL for a NULL list), Index (ContainerIndex, :300-307; 0-based, NULL
outside the list, a negative index included), InList (In with a list-valued right-hand side,
array_contains, :138-145; three-valued) over a list column, and Range (:243-245; the reference's
rangeUdf, inclusive bounds, NULL when an operand is NULL, step 0 an error), which
``GpuTable.withColumns`` turns into a list column (``capsmi_with_range_column``).

Entity functions (:192-227): Labels and Keys, String lists built on the device from flag and property columns
(``capsmi_with_mask_list_column``), and RelType, a Case over the type flags; startNode / endNode are the
relationship's source and target columns.

String matching (:152-157): StartsWith, EndsWith and Contains over String operands, matched byte-wise on the
device against the session's string store (``Session.sync_strings``).

Numeric functions: Divide (:186, ``BinOp("/")``), Sqrt / Log / Log10 / Exp / Abs / Ceil / Floor / Round / Sign
(:249-260), ToFloat and ToInteger over numbers (:229-231), and ``E`` (:253), the literal ``Math.E``.  A NULL operand
gives NULL; the rules are those of the Spark 2.2.1 Column calls the mapper makes (include/capsmi.h, CAPSMI_X_DIV ..
CAPSMI_X_TO_INTEGER).

Functions of a String's characters: StrSize (:124-127), StrToInteger (:231), StrToFloat (:229) and ToBoolean (:235),
computed on the device from the bytes of the session's string store (include/capsmi.h, CAPSMI_X_STR_SIZE ..
CAPSMI_X_TO_BOOLEAN).  The front end picks them by the operand's Cypher type; Size, ToInteger and ToFloat stay the
list and number forms.

Functions that make a String: ToString (:233) of a Long, a Boolean or a String, and Concat (Add over a String and a
String or a Number, :160-181, ``functions.concat``).  The strings are made on the device and get their codes from the
session's dictionary through the string sink (include/capsmi.h, CAPSMI_X_TO_STRING, CAPSMI_X_CONCAT,
capsmi_session_set_string_sink).  ``BinOp("+")`` compiles to the concatenation when an operand is typed String by
the tree itself -- a String literal, a ToString, a Concat, a RelType, or a ``+`` over one; over a String column the
front end builds ``Concat``, as it picks ``StrSize`` for ``Size``.  Double operands are not implemented.

MonotonicallyIncreasingId (:189) is the row's index (include/capsmi.h, CAPSMI_X_ROW_ID): the one expression the
planner emits that is not a function of the row's values.

``compile_program`` lowers a tree to the postfix ``capsmi_expr`` program of include/capsmi.h.
"""
from __future__ import annotations

import ctypes
import math
import struct
from dataclasses import dataclass
from typing import Callable, Sequence, Tuple, Union

# physical types (include/capsmi.h)
I64, BOOL, F64, STR = 0, 1, 2, 3
LIST = 8  # list column of element type t: LIST + t (include/capsmi.h CAPSMI_LIST_*; Collect results)
TYPE_NAMES = {I64: "I64", BOOL: "BOOL", F64: "F64", STR: "STR"}

# expression opcodes (include/capsmi.h CAPSMI_X_*)
X_COL, X_LIT, X_NULL, X_EQ, X_NEQ, X_LT, X_LE, X_GT, X_GE, X_NOT, X_AND, X_OR = range(12)
X_ISNULL, X_ISNOTNULL, X_IN, X_ADD, X_SUB, X_MUL, X_NEG, X_COALESCE = range(12, 20)
X_BITAND, X_BITOR, X_SHL, X_SHRU, X_CASE, X_PARAM = range(20, 26)
X_SIZE, X_INDEX, X_IN_LIST = range(26, 29)  # list operands: a Col of a list column
X_STARTS_WITH, X_ENDS_WITH, X_CONTAINS = range(29, 32)  # String operands; they read the session's string store
STRING_MATCH_OPS = (X_STARTS_WITH, X_ENDS_WITH, X_CONTAINS)
# 32..39 are unassigned; the numeric block starts at 40
(X_DIV, X_SQRT, X_LOG, X_LOG10, X_EXP, X_ABS, X_CEIL, X_FLOOR, X_ROUND, X_SIGN, X_TO_FLOAT,
 X_TO_INTEGER) = range(40, 52)
# 52..55 are unassigned; the functions that read a String's characters (they read the session's string store too)
X_STR_SIZE, X_STR_TO_INTEGER, X_STR_TO_FLOAT, X_TO_BOOLEAN = range(56, 60)
STRING_CONV_OPS = (X_STR_SIZE, X_STR_TO_INTEGER, X_STR_TO_FLOAT, X_TO_BOOLEAN)
# 60..63 are unassigned; the functions that make a String: their codes come from the session's string sink
X_TO_STRING, X_CONCAT = 64, 65
STRING_MAKE_OPS = (X_TO_STRING, X_CONCAT)
# 66..67 are unassigned; the row's index: legal only in a withColumns program, whose plan node it pins
X_ROW_ID = 68
STRING_STORE_OPS = STRING_MATCH_OPS + STRING_CONV_OPS  # the opcodes that read a String's bytes
# a program that holds one needs Session.sync_strings(): the makers read STR operands from the store and merge into it
STRING_SYNC_OPS = STRING_STORE_OPS + STRING_MAKE_OPS

BIN_OPS = {"=": X_EQ, "<>": X_NEQ, "<": X_LT, "<=": X_LE, ">": X_GT, ">=": X_GE, "+": X_ADD, "-": X_SUB, "*": X_MUL,
           "/": X_DIV, "&": X_BITAND, "|": X_BITOR, "<<": X_SHL, ">>>": X_SHRU}


class Expr:
    """Base class; trees are immutable value objects."""

    # small builder conveniences so planner code reads like Cypher
    def __eq__(self, other):  # type: ignore[override]
        return type(self) is type(other) and self.__dict__ == other.__dict__

    def __hash__(self):
        return hash((type(self).__name__, repr(self)))


@dataclass(frozen=True, eq=False)
class Col(Expr):
    name: str


@dataclass(frozen=True, eq=False)
class Lit(Expr):
    """A literal.  ``value`` is a Python int / bool / float / str (strings are dictionary-encoded
    by the session before reaching the device) or None for NULL."""
    value: object
    type: int = -1

    def resolved_type(self) -> int:
        if self.type >= 0:
            return self.type
        v = self.value
        if isinstance(v, bool):
            return BOOL
        if isinstance(v, int):
            return I64
        if isinstance(v, float):
            return F64
        if isinstance(v, str):
            return STR
        return -1


@dataclass(frozen=True, eq=False)
class BinOp(Expr):
    op: str
    left: Expr
    right: Expr


@dataclass(frozen=True, eq=False)
class Not(Expr):
    arg: Expr


@dataclass(frozen=True, eq=False)
class Neg(Expr):
    arg: Expr


@dataclass(frozen=True, eq=False)
class Ands(Expr):
    args: Tuple[Expr, ...]


@dataclass(frozen=True, eq=False)
class Ors(Expr):
    args: Tuple[Expr, ...]


@dataclass(frozen=True, eq=False)
class IsNull(Expr):
    arg: Expr


@dataclass(frozen=True, eq=False)
class IsNotNull(Expr):
    arg: Expr


@dataclass(frozen=True, eq=False)
class In(Expr):
    arg: Expr
    values: Tuple[Expr, ...]


@dataclass(frozen=True, eq=False)
class Coalesce(Expr):
    args: Tuple[Expr, ...]


@dataclass(frozen=True, eq=False)
class Case(Expr):
    """CaseExpr (okapi-ir Expr.scala; SparkSQLExprMapper.scala:283-298): the value of the first
    alternative whose predicate is TRUE, else ``default`` (NULL when None)."""
    alternatives: Tuple[Tuple[Expr, Expr], ...]
    default: object = None


@dataclass(frozen=True, eq=False)
class Param(Expr):
    """Param(name) (okapi-ir Expr.scala): query parameter ``index`` of the session's parameter table
    (``Session.set_params``), bound to a literal by the library when the program is handed over, as
    SparkSQLExprMapper.scala:86-92 turns it into ``functions.lit``.  A list parameter may only be an
    element of ``In``, where it stands for its values."""
    index: int


@dataclass(frozen=True, eq=False)
class ListLit(Expr):
    """ListLit (okapi-ir Expr.scala; SparkSQLExprMapper.scala:111-112, functions.array of the literals):
    Python scalars (int, float, bool, str, None) of one type.  On the device path it is the operand of
    ``Explode`` only."""
    values: Tuple[object, ...]


@dataclass(frozen=True, eq=False)
class Explode(Expr):
    """Explode(list) (okapi-ir Expr.scala; SparkSQLExprMapper.scala:237-241, functions.explode): what
    RelationalPlanner.scala:94-96 adds for UNWIND.  ``arg`` is a list column (``Col``), a ``ListLit`` or a
    list ``Param``.  Only the whole expression of one ``withColumns`` column may be an Explode, and one per
    call (Spark allows one generator per select)."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Size(Expr):
    """Size(list) (SparkSQLExprMapper.scala:124-130): the element count of a list column; NULL for a NULL
    list.  ``size()`` of a string is not implemented on the device path."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Index(Expr):
    """ContainerIndex(list, index) (SparkSQLExprMapper.scala:300-307, Spark's GetArrayItem): element
    ``index`` (0-based, a Long expression) of a list column; NULL when the list or the index is NULL or
    the index lies outside the list -- a negative index does not count from the end."""
    list: Expr
    index: Expr


@dataclass(frozen=True, eq=False)
class InList(Expr):
    """In(arg, list) with a list-valued right-hand side (SparkSQLExprMapper.scala:138-145,
    array_contains): NULL when ``arg`` or the list is NULL, TRUE when some element equals ``arg`` under
    ``=``, NULL when the element type cannot be compared with ``arg``'s, else FALSE.  With a ``ListLit``
    or a list ``Param`` on the right it is the plain ``In``."""
    arg: Expr
    list: Expr


@dataclass(frozen=True, eq=False)
class Range(Expr):
    """Range(start, end, step) (SparkSQLExprMapper.scala:243-245; CAPSFunctions.scala:50 rangeUdf, Scala's
    ``start.to(end, step)``): the Long list start, start + step, ... up to and including ``end``; empty
    when ``end`` lies on the wrong side; NULL when an operand is NULL; step 0 fails the query.  ``step``
    None is 1.  Allowed as a whole ``withColumns`` column, as the argument of ``Explode`` and as the list
    of ``Size`` / ``Index`` / ``InList``."""
    start: Expr
    end: Expr
    step: object = None


@dataclass(frozen=True, eq=False)
class StartsWith(Expr):
    """StartsWith(lhs, rhs) (okapi-ir Expr.scala; SparkSQLExprMapper.scala:152-153, ``Column.startsWith``, Spark's
    ``UTF8String.startsWith``): whether the String ``arg`` begins with the String ``pattern``, compared byte by byte
    over UTF-8.  NULL when either operand is NULL (ExpressionBehaviour.scala:768-784); the empty pattern matches
    every non-null string.  Both operands are String expressions (or a NULL literal)."""
    arg: Expr
    pattern: Expr


@dataclass(frozen=True, eq=False)
class EndsWith(Expr):
    """EndsWith(lhs, rhs) (SparkSQLExprMapper.scala:154-155, ``Column.endsWith``, ``UTF8String.endsWith``): whether
    ``arg`` ends with ``pattern``; NULL when either operand is NULL (ExpressionBehaviour.scala:808-824)."""
    arg: Expr
    pattern: Expr


@dataclass(frozen=True, eq=False)
class Contains(Expr):
    """Contains(lhs, rhs) (SparkSQLExprMapper.scala:156-157, ``Column.contains``, ``UTF8String.contains``): whether
    ``pattern`` occurs in ``arg`` as a run of bytes (UTF-8 is self-synchronising, so this is a run of characters);
    NULL when either operand is NULL (ExpressionBehaviour.scala:848-864)."""
    arg: Expr
    pattern: Expr


_STRING_MATCH = {StartsWith: X_STARTS_WITH, EndsWith: X_ENDS_WITH, Contains: X_CONTAINS}


@dataclass(frozen=True, eq=False)
class Sqrt(Expr):
    """Sqrt(expr) (SparkSQLExprMapper.scala:249, ``functions.sqrt``): the correctly rounded square root as a Double;
    a Long operand is converted first.  A negative operand gives NaN, not NULL; NULL gives NULL."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Log(Expr):
    """Log(expr) (SparkSQLExprMapper.scala:250, ``functions.log``): the natural logarithm as a Double; NULL when the
    operand is NULL or <= 0 (Spark's UnaryLogExpression), NaN for NaN."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Log10(Expr):
    """Log10(expr) (SparkSQLExprMapper.scala:251, ``functions.log(10.0, expr)``, Spark's Logarithm):
    ``log(x) / log(10.0)``, not ``log10(x)`` -- log10(1000) is 2.9999999999999996; NULL when the operand is NULL
    or <= 0."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Exp(Expr):
    """Exp(expr) (SparkSQLExprMapper.scala:252, ``functions.exp``): e to the operand, a Double."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Abs(Expr):
    """Abs(expr) (SparkSQLExprMapper.scala:254, ``functions.abs``): of the operand's type; Long wraps
    (abs(Long.MIN) = Long.MIN), Double clears the sign bit."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Ceil(Expr):
    """Ceil(expr) (SparkSQLExprMapper.scala:255, ``functions.ceil(..).cast(DoubleType)``): Spark's Ceil yields a Long
    that the mapper casts back, so the Double result is saturated to the Long range, NaN gives 0.0 and a zero is
    +0.0."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Floor(Expr):
    """Floor(expr) (SparkSQLExprMapper.scala:256, ``functions.floor(..).cast(DoubleType)``): as Ceil."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Round(Expr):
    """Round(expr) (SparkSQLExprMapper.scala:258, ``functions.round``): to an integral Double, halves away from zero
    (HALF_UP); NaN and the infinities stay; a zero result is +0.0."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Sign(Expr):
    """Sign(expr) (SparkSQLExprMapper.scala:259, ``functions.signum(..).cast(IntegerType)``): the Long -1, 0 or 1;
    NaN and both zeros give 0."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class ToFloat(Expr):
    """ToFloat(expr) (SparkSQLExprMapper.scala:229, ``cast(DoubleType)``) of a number: a Long is converted (round to
    nearest), a Double stays.  String operands are not implemented on the device path."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class ToInteger(Expr):
    """ToInteger(expr) (SparkSQLExprMapper.scala:231, ``cast(IntegerType)``, 32 bits) of a number, held as a Long: the
    low 32 bits of a Long, sign-extended; a Double truncated toward zero and saturated to the Int range, NaN 0.
    String operands are not implemented on the device path."""
    arg: Expr


_MATH_FUNCS = {Sqrt: X_SQRT, Log: X_LOG, Log10: X_LOG10, Exp: X_EXP, Abs: X_ABS, Ceil: X_CEIL, Floor: X_FLOOR,
               Round: X_ROUND, Sign: X_SIGN, ToFloat: X_TO_FLOAT, ToInteger: X_TO_INTEGER}


@dataclass(frozen=True, eq=False)
class StrSize(Expr):
    """Size(expr) of a String (SparkSQLExprMapper.scala:124-127, ``functions.length``, Spark's
    ``UTF8String.numChars``): the number of code points as a Long -- the bytes of the UTF-8 text that are not
    ``10xxxxxx``, so an astral character counts 1.  NULL gives NULL.  The front end picks this class for an operand
    of Cypher type String and ``Size`` for a list, as the mapper's own Size does."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class StrToInteger(Expr):
    """ToInteger(expr) of a String (SparkSQLExprMapper.scala:231, ``cast(IntegerType)``, Spark's
    ``UTF8String.toInt``), held as a Long.  No trimming; the text must match ``[+-]?[0-9]*(\\.[0-9]*)?`` and be none
    of "", "+", "-"; the fraction is checked, then dropped ("82.9" gives 82, "." gives 0); the signed integer part
    must lie in [-2^31, 2^31 - 1].  Anything else -- an exponent, a blank, a value out of range -- is NULL."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class StrToFloat(Expr):
    """ToFloat(expr) of a String (SparkSQLExprMapper.scala:229, ``cast(DoubleType)``, Java's
    ``Double.parseDouble``): bytes <= 0x20 are trimmed, then an optional sign and one of ``NaN`` / ``Infinity``, a
    decimal with an optional exponent, or a hex float with its mandatory ``p`` exponent, each of the last two with
    an optional suffix out of ``fFdD``.  The Double is correctly rounded (ties to even; subnormals, overflow to an
    infinity and underflow to a zero included) for digit strings of any length.  Anything else is NULL."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class ToBoolean(Expr):
    """ToBoolean(expr) (SparkSQLExprMapper.scala:235, ``cast(BooleanType)``, Spark's ``StringUtils.isTrueString`` /
    ``isFalseString``).  Of a String: no trimming, ASCII case folded; "t", "true", "y", "yes", "1" give TRUE, "f",
    "false", "n", "no", "0" FALSE, anything else NULL.  Of a Boolean: the operand itself."""
    arg: Expr


_STRING_CONV = {StrSize: X_STR_SIZE, StrToInteger: X_STR_TO_INTEGER, StrToFloat: X_STR_TO_FLOAT, ToBoolean: X_TO_BOOLEAN}


@dataclass(frozen=True, eq=False)
class ToString(Expr):
    """ToString(expr) (SparkSQLExprMapper.scala:233, ``cast(StringType)``).  Of a Long: Java's ``Long.toString`` --
    decimal digits, a leading ``-`` for a negative value, no ``+``, no padding.  Of a Boolean: ``true`` or ``false``.  Of
    a String: the operand itself.  NULL gives NULL.  A Double operand is not implemented on the device path (Java's
    ``Double.toString`` is not restated)."""
    arg: Expr


@dataclass(frozen=True, eq=False)
class Concat(Expr):
    """Add(lhs, rhs) over a String and a String or a Long (SparkSQLExprMapper.scala:160-181, ``functions.concat``, the
    Long cast to StringType): the bytes of ``left`` followed by the bytes of ``right``; NULL when either is NULL.  At
    least one operand is a String; a Boolean or a Double operand is refused."""
    left: Expr
    right: Expr


@dataclass(frozen=True, eq=False)
class MonotonicallyIncreasingId(Expr):
    """MonotonicallyIncreasingId() (SparkSQLExprMapper.scala:189, ``functions.monotonically_increasing_id()``): the
    0-based index of the row in the table the ``withColumns`` reads, Spark's value for a single partition -- what
    ``ConstructGraphPlanner.generateId`` builds the ids of created entities from (include/capsmi.h, CAPSMI_X_ROW_ID).
    A Long, never NULL.  Legal only in ``withColumns``; the plan node is pinned: computed whole and once, no filter
    pushed below it, its rows kept for every later reader."""


def is_string_typed(e: Expr) -> bool:
    """Whether the tree itself types ``e`` as a String (a column's type is the front end's to know)."""
    if isinstance(e, Lit):
        return e.resolved_type() == STR
    if isinstance(e, (ToString, Concat, RelType)):
        return True
    return isinstance(e, BinOp) and e.op == "+" and (is_string_typed(e.left) or is_string_typed(e.right))


def _sorted_by_name(cols, names):
    cols, names = tuple(cols), tuple(names)
    if len(cols) != len(names):
        raise ValueError(f"{len(cols)} columns for {len(names)} names")
    order = sorted(range(len(names)), key=lambda i: names[i])
    return tuple(cols[i] for i in order), tuple(names[i] for i in order)


@dataclass(frozen=True, eq=False)
class Labels(Expr):
    """Labels(node) (SparkSQLExprMapper.scala:192-201; CAPSFunctions.scala:73-81 get_node_labels): the String
    list of the ``names`` whose Boolean flag column is TRUE, in name order (``sortBy(_._1)``, :198 -- sorted
    here, whatever order is given).  A NULL flag is not set, so a null node (an OPTIONAL MATCH miss) gives
    ``[]``, never NULL: a reading of filterWithMask's ``case (label, true)``, not an observation of a run.
    Allowed where a ``Range`` is: a whole ``withColumns`` column, the argument of ``Explode`` and the list of
    ``Size`` / ``Index`` / ``InList`` (``capsmi_with_mask_list_column``, CAPSMI_MASK_TRUE)."""
    flag_cols: Tuple[str, ...]
    names: Tuple[str, ...]

    def __post_init__(self):
        cols, names = _sorted_by_name(self.flag_cols, self.names)
        object.__setattr__(self, "flag_cols", cols)
        object.__setattr__(self, "names", names)


@dataclass(frozen=True, eq=False)
class Keys(Expr):
    """Keys(entity) (SparkSQLExprMapper.scala:203-208; CAPSFunctions.scala:83-91 get_property_keys): the String
    list of the ``names`` whose property column is not NULL in the row, in key order (``sortBy(_.key.name)``,
    :205 -- sorted here).  Columns of any type, list columns included; never NULL (a null entity gives ``[]``,
    read from filterNotNull's ``value != null``).  Allowed where a ``Labels`` is (CAPSMI_MASK_NOT_NULL)."""
    cols: Tuple[str, ...]
    names: Tuple[str, ...]

    def __post_init__(self):
        cols, names = _sorted_by_name(self.cols, self.names)
        object.__setattr__(self, "cols", cols)
        object.__setattr__(self, "names", names)


@dataclass(frozen=True, eq=False)
class RelType(Expr):
    """Type(rel) over relationship-type flag columns (SparkSQLExprMapper.scala:210-219; CAPSFunctions.scala:68-71
    get_rel_type, ``headOption.orNull``): the name of the first TRUE flag in the order given (the reference does
    not sort the types), NULL when none is.  Compiled as the ``Case`` of ``to_case``; no kernel of its own."""
    flag_cols: Tuple[str, ...]
    names: Tuple[str, ...]

    def __post_init__(self):
        object.__setattr__(self, "flag_cols", tuple(self.flag_cols))
        object.__setattr__(self, "names", tuple(self.names))
        if len(self.flag_cols) != len(self.names):
            raise ValueError(f"{len(self.flag_cols)} columns for {len(self.names)} names")

    def to_case(self) -> "Case":
        return Case(tuple((Col(c), Lit(n)) for c, n in zip(self.flag_cols, self.names)), Lit(None, STR))


MASK_TRUE, MASK_NOT_NULL = 0, 1  # include/capsmi.h CAPSMI_MASK_*


def mask_list_args(e: Expr):
    """(mode, columns, names) of a Labels / Keys for ``GpuTable.withMaskListColumn``."""
    if isinstance(e, Labels):
        return MASK_TRUE, e.flag_cols, e.names
    if isinstance(e, Keys):
        return MASK_NOT_NULL, e.cols, e.names
    raise TypeError(f"not a Labels / Keys: {e!r}")


def _children(e: Expr):
    for v in e.__dict__.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            for y in (x if isinstance(x, tuple) else (x,)):  # Case alternatives are pairs
                if isinstance(y, Expr):
                    yield y


def contains_range(e: Expr) -> bool:
    """Whether a Range occurs anywhere in ``e``."""
    return isinstance(e, Range) or any(contains_range(c) for c in _children(e))


def needs_list_lowering(e: Expr) -> bool:
    """Whether ``GpuTable`` has to rewrite ``e`` before compiling it: a Range, a Labels, a Keys, a Size or an
    InList occurs, or an Index of a literal."""
    if isinstance(e, (Range, Labels, Keys, Size, InList)) or (isinstance(e, Index) and isinstance(e.list, (ListLit, Lit))):
        return True
    return any(needs_list_lowering(c) for c in _children(e))


def contains_explode(e: Expr) -> bool:
    """Whether an Explode occurs anywhere in ``e``."""
    if isinstance(e, Explode):
        return True
    for v in e.__dict__.values():
        for x in (v if isinstance(v, tuple) else (v,)):
            for y in (x if isinstance(x, tuple) else (x,)):  # Case alternatives are pairs
                if isinstance(y, Expr) and contains_explode(y):
                    return True
    return False


TRUE = Lit(True)
FALSE = Lit(False)
NULL = Lit(None)
E = Lit(math.e)  # E() (SparkSQLExprMapper.scala:253, functions.lit(Math.E)): no opcode


def eq(a: Expr, b: Expr) -> Expr:
    return BinOp("=", a, b)


def ands(*args: Expr) -> Expr:
    flat = []
    for a in args:
        if isinstance(a, Ands):
            flat.extend(a.args)
        elif not (isinstance(a, Lit) and a.value is True):
            flat.append(a)
    if not flat:
        return TRUE
    return flat[0] if len(flat) == 1 else Ands(tuple(flat))


def columns_of(e: Expr) -> set:
    """Physical columns an expression reads."""
    if isinstance(e, Col):
        return {e.name}
    if isinstance(e, (Labels, RelType)):
        return set(e.flag_cols)
    if isinstance(e, Keys):
        return set(e.cols)
    out = set()
    for v in e.__dict__.values():
        if isinstance(v, Expr):
            out |= columns_of(v)
        elif isinstance(v, tuple):
            for x in v:
                if isinstance(x, Expr):
                    out |= columns_of(x)
                elif isinstance(x, tuple):  # Case alternatives
                    for y in x:
                        out |= columns_of(y)
    return out


class CapsmiExpr(ctypes.Structure):
    _fields_ = [("op", ctypes.c_int32), ("arg", ctypes.c_int32), ("type", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("ival", ctypes.c_int64)]


def _lit_bits(value, ty: int, encode_str: Callable[[str], int]) -> int:
    if ty == BOOL:
        return 1 if value else 0
    if ty == I64:
        v = int(value)
        if not -(1 << 63) <= v < (1 << 63):
            raise OverflowError("integer literal outside Long range")
        return v
    if ty == F64:
        return struct.unpack("<q", struct.pack("<d", float(value)))[0]
    if ty == STR:
        return encode_str(value)
    raise ValueError(f"literal type {ty}")


def compile_program(e: Expr, column_index: Callable[[str], int], encode_str: Callable[[str], int]):
    """Postfix program (list of (op, arg, type, ival)) for ``e``."""
    out = []

    def go(x: Expr):
        if isinstance(x, Col):
            out.append((X_COL, column_index(x.name), 0, 0))
        elif isinstance(x, Lit):
            ty = x.resolved_type()
            if x.value is None or ty < 0:
                out.append((X_NULL, x.type + 1 if x.type >= 0 else 0, 0, 0))
            else:
                out.append((X_LIT, 0, ty, _lit_bits(x.value, ty, encode_str)))
        elif isinstance(x, Param):
            out.append((X_PARAM, x.index, 0, 0))
        elif isinstance(x, MonotonicallyIncreasingId):
            out.append((X_ROW_ID, 0, 0, 0))
        elif isinstance(x, BinOp):
            go(x.left)
            go(x.right)
            out.append((X_CONCAT if x.op == "+" and is_string_typed(x) else BIN_OPS[x.op], 0, 0, 0))
        elif isinstance(x, Not):
            go(x.arg)
            out.append((X_NOT, 0, 0, 0))
        elif isinstance(x, Neg):
            go(x.arg)
            out.append((X_NEG, 0, 0, 0))
        elif isinstance(x, (Ands, Ors)):
            if not x.args:
                out.append((X_LIT, 0, BOOL, 1 if isinstance(x, Ands) else 0))
                return
            for a in x.args:
                go(a)
            out.append((X_AND if isinstance(x, Ands) else X_OR, len(x.args), 0, 0))
        elif isinstance(x, IsNull):
            go(x.arg)
            out.append((X_ISNULL, 0, 0, 0))
        elif isinstance(x, IsNotNull):
            go(x.arg)
            out.append((X_ISNOTNULL, 0, 0, 0))
        elif isinstance(x, In):
            go(x.arg)
            for v in x.values:
                go(v)
            out.append((X_IN, len(x.values), 0, 0))
        elif isinstance(x, Coalesce):
            for a in x.args:
                go(a)
            out.append((X_COALESCE, len(x.args), 0, 0))
        elif isinstance(x, Size):
            go(x.arg)
            out.append((X_SIZE, 0, 0, 0))
        elif isinstance(x, Index):
            go(x.list)
            go(x.index)
            out.append((X_INDEX, 0, 0, 0))
        elif isinstance(x, InList):
            go(x.arg)
            go(x.list)
            out.append((X_IN_LIST, 0, 0, 0))
        elif type(x) in _STRING_MATCH:
            go(x.arg)
            go(x.pattern)
            out.append((_STRING_MATCH[type(x)], 0, 0, 0))
        elif type(x) in _MATH_FUNCS:
            go(x.arg)
            out.append((_MATH_FUNCS[type(x)], 0, 0, 0))
        elif type(x) in _STRING_CONV:
            go(x.arg)
            out.append((_STRING_CONV[type(x)], 0, 0, 0))
        elif isinstance(x, ToString):
            go(x.arg)
            out.append((X_TO_STRING, 0, 0, 0))
        elif isinstance(x, Concat):
            go(x.left)
            go(x.right)
            out.append((X_CONCAT, 0, 0, 0))
        elif isinstance(x, RelType):
            go(x.to_case())
        elif isinstance(x, Case):
            if not x.alternatives:
                go(x.default if x.default is not None else NULL)
                return
            for p, v in x.alternatives:
                go(p)
                go(v)
            go(x.default if x.default is not None else NULL)
            out.append((X_CASE, len(x.alternatives), 0, 0))
        else:
            raise NotImplementedError(f"expression {x!r}")

    go(e)
    return out


def to_ctypes(prog: Sequence[Tuple[int, int, int, int]]):
    arr = (CapsmiExpr * max(1, len(prog)))()
    for i, (op, arg, ty, ival) in enumerate(prog):
        arr[i].op, arr[i].arg, arr[i].type, arr[i].ival = op, arg, ty, ival
    return arr


ExprLike = Union[Expr, str]
