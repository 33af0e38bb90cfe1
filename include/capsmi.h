/*
 * capsmi.h -- C ABI of the MI355X execution backend for CAPS pattern matching.
 *
 * This is the drop-in boundary.  In CAPS the backend plug-in
 * point is the Scala trait
 *     trait Table[T <: Table[T]] extends CypherTable
 *     okapi-relational/src/main/scala/org/opencypher/okapi/relational/api/table/Table.scala:43-176
 * implemented for Spark by DataFrameTable
 *     spark-cypher/src/main/scala/org/opencypher/spark/impl/table/SparkTable.scala:47-257
 * A JVM shim (`GpuTable extends Table[GpuTable]`) binds each
 * method below over JNI.  Every entry point cites the Scala member it replaces.
 *
 * Conventions
 *  - Every call returns capsmi_status (0 = OK).  On failure capsmi_last_error()
 *    returns a thread-local message.  The shim maps the codes to the okapi
 *    exception classes (okapi-api/.../impl/exception/InternalException.scala:34-59).
 *  - Handles are opaque and reference counted.  Tables are immutable: every op
 *    returns a NEW table and never modifies its inputs (Table.scala: each op
 *    returns T; inputs stay valid for DAG sharing / cached sub-trees).
 *  - Columns are addressed by name, as in Table.scala (`cols: String*`).
 *  - Values are 8 bytes per row: I64 (Spark LongType), BOOL (0/1), F64 (bits of
 *    an IEEE double), STR (order-preserving dictionary code assigned by the
 *    caller; equal strings <=> equal codes, string order <=> code order).
 *    Nullability is a byte per row (1 = valid), or absent when a column has no nulls.
 *  - A session is externally synchronised (one caller thread, like a CAPS
 *    driver) and owns one HIP stream on one gfx950 device.  Device work is
 *    stream-ordered; calls that return a size to the host synchronise.  Caller
 *    device buffers (ext words, owned_in, dev_out, ...) are read and written in
 *    the session stream's order only: the host orders its own writes to them
 *    before the call (one stream, or an event the session stream waits on).
 */
#ifndef CAPSMI_H
#define CAPSMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------- */
typedef int32_t capsmi_status;
enum {
    CAPSMI_OK = 0,
    CAPSMI_ERR_ILLEGAL_ARGUMENT = 1, /* okapi IllegalArgumentException */
    CAPSMI_ERR_NOT_IMPLEMENTED = 2,  /* okapi NotImplementedException */
    CAPSMI_ERR_UNSUPPORTED = 3,      /* okapi UnsupportedOperationException */
    CAPSMI_ERR_DEVICE = 4,           /* HIP runtime error (no GPU, fault, ...) */
    CAPSMI_ERR_OUT_OF_MEMORY = 5,
    CAPSMI_ERR_INTERNAL = 6          /* okapi InternalException */
};

/* ---- handles ----------------------------------------------------------------- */
typedef struct capsmi_session capsmi_session;
typedef struct capsmi_table capsmi_table;
typedef struct capsmi_bitmap capsmi_bitmap;

/* ---- value types (CypherType -> physical type, SparkConversions.scala:55-168) -- */
enum {
    CAPSMI_I64 = 0,  /* CTInteger, CTNode/CTRelationship ids (Long) */
    CAPSMI_BOOL = 1, /* CTBoolean, label / rel-type flag columns */
    CAPSMI_F64 = 2,  /* CTFloat */
    CAPSMI_STR = 3   /* CTString, dictionary code */
};

/* List columns (CTList(elem)): the result of a Collect aggregator (SparkTable.scala:169-177,
 * functions.sort_array(collect_list / collect_set)).  The column type is CAPSMI_LIST + element type
 * (CAPSMI_LIST_I64 ... CAPSMI_LIST_STR); rows are read with capsmi_table_export_list, opened again into
 * rows by capsmi_explode, and ingested from the host by capsmi_table_add_list_column.  List columns
 * travel through select / drop / rename / filter / join payloads / union all / order-by payloads /
 * skip / limit, and are made from Long operands by capsmi_with_range_column and from flag or property
 * columns by capsmi_with_mask_list_column.  Inside an expression a list
 * column is an operand of CAPSMI_X_SIZE, CAPSMI_X_INDEX and CAPSMI_X_IN_LIST only: CAPSMI_X_COL of a list
 * column pushes a list value (the row's list, typed CAPSMI_LIST + elem, or NULL for a null row), and a list
 * value that reaches any other opcode is CAPSMI_ERR_NOT_IMPLEMENTED, as is a list column used as a join,
 * grouping, distinct or sort key. */
enum {
    CAPSMI_LIST = 8,
    CAPSMI_LIST_I64 = 8,
    CAPSMI_LIST_BOOL = 9,
    CAPSMI_LIST_F64 = 10,
    CAPSMI_LIST_STR = 11
};

/* Input-only value widths of capsmi_col_desc.type: widened at ingest the way
 * DataFrameOps.withCypherCompatibleTypes lifts Spark columns (spark-cypher/.../impl/DataFrameOps.scala:185-198,
 * SparkConversions.scala:162-168): Byte/Short/Integer -> Long, Float -> Double; a Boolean byte -> BOOL. */
enum {
    CAPSMI_IN_I32 = 16,  /* int32  -> CAPSMI_I64 */
    CAPSMI_IN_I16 = 17,  /* int16  -> CAPSMI_I64 */
    CAPSMI_IN_I8 = 18,   /* int8   -> CAPSMI_I64 */
    CAPSMI_IN_F32 = 19,  /* float  -> CAPSMI_F64 */
    CAPSMI_IN_BOOL8 = 20 /* uint8 0/1 -> CAPSMI_BOOL */
};

typedef struct {
    const char* name;
    int32_t type;         /* CAPSMI_I64 ... CAPSMI_STR, or a CAPSMI_IN_* width */
    const void* data;     /* nrows x 8 bytes (nrows x the CAPSMI_IN_* width) */
    const uint8_t* valid; /* nrows bytes (1 = non-null) or NULL (no nulls) */
} capsmi_col_desc;

/* ---- expressions: postfix programs over one row -------------------------------
 * Subset of SparkSQLExprMapper.asSparkSQLExpr (spark-cypher/.../impl/SparkSQLExprMapper.scala:81-312)
 * that the pattern-matching path needs: column refs (Var/Property/HasLabel/HasType/StartNode/EndNode
 * resolve to columns, :97-105), literals and params (:86-92, :111-117), Equals (:120), Not (:121),
 * IsNull/IsNotNull (:122-123), Ands/Ors (:132-136), In (:138-145), < <= > >= (:147-150), arithmetic.
 * Evaluation follows SQL three-valued logic; Filter keeps rows whose value is TRUE.
 * Static types: a column or literal has its own, an untyped NULL none, comparisons and predicates are BOOL.
 * CAPSMI_X_COALESCE and CAPSMI_X_CASE take the type of their first typed alternative (CASE: v1 .. v_arg, then
 * the default); that is the type of a column computed from one.  Where the typed alternatives disagree the
 * value is "mixed", as is + - * / NEG or ABS over it: accepted as a value or a comparison operand, but
 * CAPSMI_ERR_ILLEGAL_ARGUMENT where one type is demanded, that is as an operand of CAPSMI_X_STARTS_WITH /
 * ENDS_WITH / CONTAINS, as the index of CAPSMI_X_INDEX, or as the list operand of a list opcode. */
enum {
    CAPSMI_X_COL = 0,      /* push column `arg` (index into the input table) */
    CAPSMI_X_LIT = 1,      /* push literal of type `type`, bits in `ival` */
    CAPSMI_X_NULL = 2,     /* push NULL; arg = 1 + declared type (0 = untyped) */
    CAPSMI_X_EQ = 3,       /* pop b, a; push a = b */
    CAPSMI_X_NEQ = 4,
    CAPSMI_X_LT = 5,
    CAPSMI_X_LE = 6,
    CAPSMI_X_GT = 7,
    CAPSMI_X_GE = 8,
    CAPSMI_X_NOT = 9,
    CAPSMI_X_AND = 10,     /* pop `arg` operands, push conjunction (3VL) */
    CAPSMI_X_OR = 11,      /* pop `arg` operands, push disjunction (3VL) */
    CAPSMI_X_ISNULL = 12,
    CAPSMI_X_ISNOTNULL = 13,
    CAPSMI_X_IN = 14,      /* stack [x, v1..v_arg]: x IN (v1..v_arg), 3VL */
    CAPSMI_X_ADD = 15,
    CAPSMI_X_SUB = 16,
    CAPSMI_X_MUL = 17,
    CAPSMI_X_NEG = 18,
    CAPSMI_X_COALESCE = 19, /* pop `arg` operands, push the first non-null */
    CAPSMI_X_BITAND = 20,   /* Long a & b (SparkSQLExprMapper.scala:264-265) */
    CAPSMI_X_BITOR = 21,    /* Long a | b (:267-268) */
    CAPSMI_X_SHL = 22,      /* Long a << (b & 63) (:270-271, functions.shiftLeft) */
    CAPSMI_X_SHRU = 23,     /* Long a >>> (b & 63) (:273-274, functions.shiftRightUnsigned) */
    CAPSMI_X_CASE = 24,     /* stack [p1, v1, .., p_arg, v_arg, default]: v_i of the first TRUE p_i, else
                               default (push a NULL for none); CaseExpr, :283-298 */
    CAPSMI_X_PARAM = 25,    /* push query parameter `arg` of the session's table (capsmi_session_set_params);
                               bound to a literal when the program enters the library, as Param(name) ->
                               functions.lit (:86-92).  A list parameter may only be an element operand of
                               IN, where it expands to its values (:86-89, functions.array) */
    /* List operands (a CAPSMI_X_COL of a CAPSMI_LIST_* column; nothing else yields a list). */
    CAPSMI_X_SIZE = 26,     /* stack [list]: Long element count; NULL for a NULL list (the bag the acceptance
                               case "size() on null" states, not Spark 2's legacy -1); Size, :124-130 */
    CAPSMI_X_INDEX = 27,    /* stack [list, i]: element i (0-based) of the element type; NULL when the list or i
                               is NULL or when i < 0 or i >= size (Spark's GetArrayItem: a negative index does
                               not count from the end); i must be Long, else CAPSMI_ERR_ILLEGAL_ARGUMENT;
                               ContainerIndex, :300-307 */
    CAPSMI_X_IN_LIST = 28,  /* stack [x, list]: BOOL, 3VL: NULL when x or the list is NULL; TRUE when some
                               element equals x under the interpreter's `=` (Long against Double as doubles,
                               NaN = NaN); NULL when the element type is not comparable with x (Long against
                               STR), as `=` gives; else FALSE (stores hold no element nulls).  In with a
                               list-valued right-hand side, array_contains, :138-145.  Each IN_LIST of a
                               program runs as one load-balanced pass over all the rows' elements before the
                               row-wise interpreter, which then reads its result as a column. */
    /* String matching (StartsWith / EndsWith / Contains, :152-157: Column.startsWith / endsWith / contains,
       Spark's UTF8String).  Stack [s, p], both CAPSMI_STR or a NULL literal (typed STR or untyped), else
       CAPSMI_ERR_ILLEGAL_ARGUMENT when the node is built (a list value: CAPSMI_ERR_NOT_IMPLEMENTED); each
       operand may be any scalar expression.  BOOL, 3VL: NULL when s or p is NULL, else TRUE or FALSE.  Bytes
       of UTF-8 are compared (UTF-8 is self-synchronising, so nothing is decoded); the empty pattern matches
       every non-null string, a pattern longer than the string never does.  The bytes come from the string
       store that is registered when the action runs (capsmi_session_set_strings): without one the action
       fails with CAPSMI_ERR_ILLEGAL_ARGUMENT ("no string store"), as it does when a non-null operand's code
       is not registered in it.  A NULL literal operand gives NULL in every row without a kernel; two constants
       are folded on the host.  Each of these nodes runs as a pass of its own before the row-wise interpreter
       (k_strmatch.hip), which then reads its result as a column; CONTAINS is load-balanced over all the
       rows' start positions. */
    CAPSMI_X_STARTS_WITH = 29, /* stack [s, p]: s STARTS WITH p */
    CAPSMI_X_ENDS_WITH = 30,   /* stack [s, p]: s ENDS WITH p */
    CAPSMI_X_CONTAINS = 31,    /* stack [s, p]: s CONTAINS p */
    /* 32..39 are unassigned: CAPSMI_ERR_NOT_IMPLEMENTED "unknown expression op N", as every other number. */
    /* Numeric functions (Divide, :186; Sqrt .. Sign, :249-260; ToFloat / ToInteger, :229-231).  A NULL operand
       gives NULL.  An operand whose static type is BOOL or STR is CAPSMI_ERR_NOT_IMPLEMENTED when the node is
       built (a list value too); an untyped NULL and a "mixed" value are accepted, and a row that holds a
       non-numeric value yields NULL, as + - * do.  A Long operand of a Double-valued function is converted to
       double first (round to nearest).  sat(d) below is Java's (long) d: 0 for NaN, Long.MAX for d >= 2^63,
       Long.MIN for d <= -2^63, else d truncated toward zero.  The rules are those of the Spark 2.2.1 Column
       calls the mapper makes, stated from knowledge of Spark's source, not from a run.  E() (:253) has no
       opcode: the front ends push the Double literal Math.E. */
    CAPSMI_X_DIV = 40,        /* stack [a, b]: both as doubles (Spark's Division coercion), p / q correctly
                                 rounded; NULL when b is zero (-0.0 and Long 0 included).  Long / Long is Long:
                                 sat(p / q), so -7 / 2 = -3, Long.MIN / -1 = Long.MAX and (2^53 + 1) / 1 = 2^53
                                 (the reference's own precision loss); any Double operand makes the result
                                 Double (mixed propagates, as for +), NaN and infinities propagate; Divide, :186 */
    CAPSMI_X_SQRT = 41,       /* stack [x]: Double sqrt(x), correctly rounded; NaN (not NULL) for x < 0, -0.0 for
                                 -0.0; functions.sqrt, :249 */
    CAPSMI_X_LOG = 42,        /* stack [x]: Double log(x); NULL when x <= 0 (UnaryLogExpression; -0.0 included),
                                 NaN for NaN; functions.log, :250 */
    CAPSMI_X_LOG10 = 43,      /* stack [x]: Double log(x) / log(10.0), the divisor the double 2.302585092994046
                                 (Spark's Logarithm, not log10: 1000 gives 2.9999999999999996); NULL when
                                 x <= 0; functions.log(10.0, e), :251 */
    CAPSMI_X_EXP = 44,        /* stack [x]: Double exp(x); functions.exp, :252 */
    CAPSMI_X_ABS = 45,        /* stack [x]: of x's type; Long wraps (abs(Long.MIN) = Long.MIN), Double clears the
                                 sign bit; functions.abs, :254 */
    CAPSMI_X_CEIL = 46,       /* stack [x]: Double (double) sat(ceil(x)): Spark's Ceil is a Long that the mapper
                                 casts back, so ceil(-0.5) = +0.0, ceil(1e300) = 2^63 and NaN gives 0.0; a Long
                                 operand is only converted; functions.ceil(e).cast(DoubleType), :255 */
    CAPSMI_X_FLOOR = 47,      /* stack [x]: Double (double) sat(floor(x)), as CEIL (floor(-0.0) = +0.0); :256 */
    CAPSMI_X_ROUND = 48,      /* stack [x]: Double round(x, 0), HALF_UP: halves away from zero; NaN and the
                                 infinities stay; a zero result is +0.0 (round(-0.4) = +0.0: BigDecimal has no
                                 signed zero); a Long operand is only converted; functions.round, :258 */
    CAPSMI_X_SIGN = 49,       /* stack [x]: Long -1, 0 or 1 (signum(double) cast to Int); NaN and both zeros give
                                 0; functions.signum(e).cast(IntegerType), :259 */
    CAPSMI_X_TO_FLOAT = 50,   /* stack [x]: Double; a Long is converted, a Double stays; cast(DoubleType), :229.
                                 String operands are not implemented */
    CAPSMI_X_TO_INTEGER = 51, /* stack [x]: Long holding Spark's 32-bit IntegerType: from Long the low 32 bits,
                                 sign-extended (2^31 gives -2^31, 2^32 + 5 gives 5); from Double truncated
                                 toward zero and saturated to [-2^31, 2^31 - 1], NaN 0; cast(IntegerType),
                                 :231.  String operands are not implemented */
    /* 52..55 are unassigned. */
    /* Functions that read a String's characters (Size of a String, :124-127, functions.length; ToFloat, :229;
       ToInteger, :231; ToBoolean, :235).  Stack [s]: CAPSMI_STR or a NULL literal (typed STR or untyped), for
       TO_BOOLEAN also BOOL; any other scalar type is CAPSMI_ERR_ILLEGAL_ARGUMENT when the node is built, as is a
       "mixed" value; a list value is CAPSMI_ERR_NOT_IMPLEMENTED.  The operand may be any scalar expression.  A
       NULL operand gives NULL.  The bytes come from the string store that is registered when the action runs
       (capsmi_session_set_strings): without one the action fails with CAPSMI_ERR_ILLEGAL_ARGUMENT ("no string
       store"), as it does when a non-null operand's code is not registered in it.  A NULL literal operand gives
       NULL in every row without a kernel; a literal operand is folded on the host.  Each of these nodes runs as
       passes of its own before the row-wise interpreter (k_strconv.hip; the parsing code is csrc/str_conv.h),
       which then reads its result as a column.  With CAPSMI_STR_MATCH = auto the conversion runs once per store
       entry and the rows look their entry up when the table has at least as many rows as the store has entries,
       else once per row; rows | dict force a side.  The rules are those of the Spark 2.2.1 calls the mapper
       makes, stated from knowledge of Spark's source, not from a run. */
    CAPSMI_X_STR_SIZE = 56,       /* stack [s]: Long, the number of code points (UTF8String.numChars): the count of
                                     bytes that are not 10xxxxxx, so an astral character counts 1 (Java's
                                     String.length would say 2).  For bytes that are not well-formed UTF-8 the
                                     result is that same count; Spark's walk by lead byte differs there.  The
                                     count is load-balanced over fixed tiles of the store's byte array */
    CAPSMI_X_STR_TO_INTEGER = 57, /* stack [s]: Long holding Spark's 32-bit IntegerType (UTF8String.toInt).  No
                                     trimming.  The bytes must match [+-]?[0-9]*(\.[0-9]*)? and be none of "",
                                     "+", "-"; the fraction is checked, then dropped ("82.9" gives 82, "-82.9"
                                     -82, ".", "+." and ".5" give 0); the signed integer part, at any number of
                                     digits, must lie in [-2^31, 2^31 - 1].  Anything else is NULL: an exponent,
                                     a blank, a second dot, a non-ASCII digit, a value out of range */
    CAPSMI_X_STR_TO_FLOAT = 58,   /* stack [s]: Double, Java's Double.parseDouble(s.toString); what throws
                                     NumberFormatException is NULL.  Bytes <= 0x20 are trimmed at both ends; an
                                     optional sign; then exactly one of: "NaN" or "Infinity" (case-sensitive; NaN
                                     is the one quiet NaN whatever the sign); a decimal D+ [.] D* or . D+ with an
                                     optional exponent [eE][+-]?D+ and an optional suffix out of fFdD; a hex float
                                     0[xX] with H+ [.] H* or . H+, a mandatory [pP][+-]?D+ and the optional suffix.
                                     The value is correctly rounded, ties to even, subnormals, overflow to
                                     +-Infinity and underflow to +-0.0 included ("-0" gives -0.0), for mantissa
                                     and exponent digit strings of any length.  Any other byte gives NULL, every
                                     non-ASCII byte among them */
    CAPSMI_X_TO_BOOLEAN = 59,     /* stack [s] or [b]: BOOL.  Of a String (StringUtils.isTrueString /
                                     isFalseString over toLowerCase): no trimming, ASCII case folded (none of the
                                     words has a non-ASCII case partner); "t", "true", "y", "yes", "1" give TRUE,
                                     "f", "false", "n", "no", "0" FALSE, anything else NULL.  Of a BOOL: the
                                     identity */
    /* 60..63 are unassigned. */
    /* Functions that make a String (ToString, :233, cast(StringType); Add over a String and a String or a Number,
       :160-181, functions.concat with the number cast to StringType).  Both yield CAPSMI_STR, which may feed any
       opcode that takes a String in the same program.  A produced String has no code until the caller gives it
       one: the action hands the strings it has made to the session's string sink (capsmi_session_set_string_sink
       below), gets their codes back and merges the new entries into the registered string store, so the codes are
       readable by every string opcode at once and by later actions.  Without a sink an action that has strings to
       make fails with CAPSMI_ERR_ILLEGAL_ARGUMENT ("no string sink").  A NULL operand gives NULL (Spark's concat is
       null if any input is); a NULL literal operand gives NULL in every row without a kernel and without a sink
       call; operands that are all literals are folded on the host, with one sink call for the one string.  A STR
       column operand reads the registered store as the string predicates do (no store, or a code that is not
       registered: CAPSMI_ERR_ILLEGAL_ARGUMENT); TO_STRING of a Long needs no store beforehand, the merge creates
       one.  An F64 operand is CAPSMI_ERR_NOT_IMPLEMENTED when the node is built: it would need Java's
       Double.toString (JDK 8's FloatingDecimal, shortest-digits output with its known anomalies), which is not
       restated here.  A list value is CAPSMI_ERR_NOT_IMPLEMENTED, a "mixed" value CAPSMI_ERR_ILLEGAL_ARGUMENT.
       Each of these nodes runs as passes of its own before the row-wise interpreter (k_strmake.hip; the formatting
       code is csrc/str_make.h): the distinct operand tuples are found first (a produced string is a function of
       its operands), one string is made per tuple, load-balanced over fixed tiles of the output bytes, and the
       rows gather their tuple's code.  a + b + c interns the intermediate a + b.  The rules are those of Spark
       2.2.1's Cast to StringType and Concat, stated from knowledge of Spark's source, not from a run. */
    CAPSMI_X_TO_STRING = 64,      /* stack [x]: STR.  Of a Long: Long.toString -- decimal digits, a leading '-' for a
                                     negative value, no '+', no padding; Long.MIN_VALUE gives the 20 bytes
                                     "-9223372036854775808".  Of a BOOL: "true" or "false".  Of a STR: the operand
                                     itself (no kernel, no sink call) */
    CAPSMI_X_CONCAT = 65,         /* stack [a, b]: STR, the bytes of a followed by the bytes of b (UTF-8 is not
                                     decoded).  Each operand is STR or I64, at least one of them STR or an untyped
                                     NULL in its place; a Long is formatted as TO_STRING does.  A BOOL operand and
                                     I64 + I64 are CAPSMI_ERR_ILLEGAL_ARGUMENT when the node is built */
    /* 66..67 are unassigned. */
    /* MonotonicallyIncreasingId (SparkSQLExprMapper.scala:189, functions.monotonically_increasing_id()), the
       expression ConstructGraphPlanner.generateId builds the ids of created entities from.  The value is the
       0-based index of the row in the table the operator reads, as that table is materialised: Spark's value for a
       single partition.  generateId's partition offset and the tag are ordinary ADD / BITAND / BITOR / SHL around
       it.  It is typed I64, so it may sit under any numeric or comparison opcode of its column's program; the nodes
       that run as passes of their own (IN_LIST, the string opcodes) keep the table's rows, so a program that holds
       one of them gives the same ids.
       Legal only in a program of capsmi_with_columns: in capsmi_filter, capsmi_with_range_column and
       capsmi_bitmap_add_scan it is CAPSMI_ERR_ILLEGAL_ARGUMENT when the node is built ("CAPSMI_X_ROW_ID ...").
       Catalyst treats the expression as nondeterministic, and so does the plan executor.  A capsmi_with_columns node
       with a ROW_ID program is pinned:
         1. no filter conjunct is pushed below it, even one that reads none of its columns;
         2. when first needed it is computed whole: all its columns, nothing pruned through it, its input evaluated
            as usual (fused routes included);
         3. it keeps its rows from then on, as capsmi_cache does, so every reader sees the same ids, in the same
            action or a later one;
         4. it is never matched as part of a fused pattern shape.
       On a session with more than one rank (capsmi_session_set_ranks) the node is CAPSMI_ERR_UNSUPPORTED when built
       ("distributed CONSTRUCT is not implemented"): Spark's (partition << 33) + row layout is not restated. */
    CAPSMI_X_ROW_ID = 68          /* stack []: I64, the row's index, never NULL; arg must be 0
                                     (CAPSMI_ERR_ILLEGAL_ARGUMENT when the node is built) */
};

typedef struct {
    int32_t op;
    int32_t arg;
    int32_t type; /* literal type for CAPSMI_X_LIT */
    int32_t reserved;
    int64_t ival; /* literal payload (int64 / 0|1 / dictionary code / double bits) */
} capsmi_expr;

typedef struct {
    const char* name;        /* output column (replaced if it exists, else appended) */
    int32_t nnodes;
    const capsmi_expr* prog;
} capsmi_expr_column;

/* ---- joins and aggregates (PhysicalConstants.scala:29-40, SparkTable.scala:121-188) ---- */
enum {
    CAPSMI_JOIN_INNER = 0,
    CAPSMI_JOIN_LEFT_OUTER = 1,
    CAPSMI_JOIN_RIGHT_OUTER = 2,
    CAPSMI_JOIN_FULL_OUTER = 3,
    CAPSMI_JOIN_CROSS = 4
};

enum {
    CAPSMI_AGG_COUNT_STAR = 0, /* count(lit 0)                  SparkTable.scala:148-149 */
    CAPSMI_AGG_COUNT = 1,      /* count / countDistinct         SparkTable.scala:152-158 */
    CAPSMI_AGG_MIN = 2,        /*                               SparkTable.scala:163-164 */
    CAPSMI_AGG_MAX = 3,        /*                               SparkTable.scala:160-161 */
    CAPSMI_AGG_SUM = 4,        /*                               SparkTable.scala:166-167 */
    CAPSMI_AGG_AVG = 5,        /* avg -> F64                    SparkTable.scala:141-146 */
    CAPSMI_AGG_COLLECT = 6     /* sort_array(collect_list) / sort_array(collect_set) when `distinct`:
                                  the group's non-null values in ascending order, a list column
                                  (an empty list for a group without values)  SparkTable.scala:169-177 */
};

typedef struct {
    int32_t kind;
    int32_t distinct;        /* COUNT only */
    const char* input;       /* input column (ignored for COUNT_STAR) */
    const char* output;      /* result column name */
} capsmi_agg;

/* ---- errors / session ----------------------------------------------------------- */
/* copies the calling thread's last error message into buf (NUL-terminated); returns its length */
size_t capsmi_last_error(char* buf, size_t n);
const char* capsmi_version(void);

/* CAPSSession.local()/create (spark-cypher/.../api/CAPSSession.scala:110-131): one device, one stream */
capsmi_status capsmi_session_create(int32_t device, capsmi_session** out);
capsmi_status capsmi_session_destroy(capsmi_session* s);
/* run subsequent work on an external hipStream_t (e.g. torch's current stream); NULL = session stream.
 * The previous stream is drained first (the session's cached device blocks then move with it); an
 * external stream must outlive the session or the next switch away from it. */
capsmi_status capsmi_session_set_stream(capsmi_session* s, void* hip_stream);
/* run subsequent work on exactly `hip_stream`; NULL = the HIP null (legacy default) stream -- what
 * torch's default stream is, so kernels and torch work stay ordered */
capsmi_status capsmi_session_use_stream(capsmi_session* s, void* hip_stream);
capsmi_status capsmi_session_sync(capsmi_session* s);
/* session configuration (ConfigOption / CoraConfiguration analogue): every CAPSMI_* knob is
 * read from the environment once, at capsmi_session_create; this changes one for this session only.
 * `name` is the knob's environment name (e.g. "CAPSMI_JOIN", "CAPSMI_COUNT"), `value` its text as the
 * environment would hold it, NULL = back to the environment's value at the time of the call (or the
 * default).  Unknown names and unparsable values are refused (CAPSMI_ERR_ILLEGAL_ARGUMENT).  The knobs and
 * their meaning: DESIGN.md §5a.  Among them CAPSMI_NARROW = auto | off: whether capsmi_rel_table (below) keeps
 * 32-bit copies of the endpoint columns and the partition's first pass reads them. */
capsmi_status capsmi_session_set_config(capsmi_session* s, const char* name, const char* value);
/* the same check without a session or device: CAPSMI_OK when capsmi_session_set_config would accept it */
capsmi_status capsmi_config_check(const char* name, const char* value);
/* per-kernel HIP-event timing of the fused graph kernels (off by default; SURVEY.md §5 tracing).
 * While enabled, each hot launch is bracketed by events on the session stream.  Enabling creates a pool of
 * events up front (resolved ones return to it), so timed queries make no event-creation calls. */
capsmi_status capsmi_session_set_profiling(capsmi_session* s, int32_t enabled);
/* which timers record while profiling is on: a comma-separated list of kernel names ("part_scatter1,hop2");
 * NULL or "" = every timer (the default).  Each timed launch adds two event records to the stream (a few
 * microseconds of device idle each), so a timed run can bracket only the launch it reports. */
capsmi_status capsmi_session_set_profiling_names(capsmi_session* s, const char* names);
/* resolve pending events (synchronises) and report totals for kernel `name` ("hop1", "hop2",
 * "expand_filter", "bitmap_add", ...; "expr_eval" is the expression interpreter, which a bitmap scan with an
 * inline range predicate does not launch): launches and summed milliseconds; then the counters reset. */
capsmi_status capsmi_session_kernel_time(capsmi_session* s, const char* name, int64_t* launches, double* total_ms);
/* summed algorithmic bytes (inputs read once, outputs written once) of the timed launches of `name`,
 * for kernels that declare them (the join kernels: "direct_join_probe", "radix_join_count",
 * "radix_join_write"; UNWIND's "explode": 8 B x (n starts + n row words read, m values read, m items + m source
 * rows written) for n input rows and m output rows, its payload gathers timed apart as "explode_gather" (24 B per
 * output row and gathered column) and its
 * lengths / scan / compaction as "explode_starts"; "explode_values": 16 B per output row;
 * capsmi_with_mask_list_column's "mask_list_len": per row 9 B per nullable and 8 B per non-nullable column read
 * under CAPSMI_MASK_TRUE, 1 B per nullable column under CAPSMI_MASK_NOT_NULL, 17 B written, and "mask_list":
 * 8 B x (n starts + n masks read, M elements written), its scan and compaction timed as "mask_list_starts";
 * string matching's "str_index", code to store index: per row 16 B, 17 B for a nullable operand, plus 8 B per
 * store entry; "str_match", the matching pass over n rows -- or over the store's entries on the dictionary side:
 * 8 B per row and column operand (its index word) + 16 B per row and operand that is not constant (two offsets) +
 * a constant pattern's bytes once + for CONTAINS 1 B per candidate slot (every start position is read at least
 * once; the bytes behind a row's last slot, a column pattern's bytes and what STARTS / ENDS WITH compare depend
 * on the data and are not counted); "str_match_lookup", the dictionary side's row gather: 18 B per row;
 * CONTAINS's lengths / scan / compaction are timed as "str_match_starts" and the row side's three-valued finish as
 * "str_match_finish", both without bytes);
 * size() / toInteger() / toFloat() / toBoolean() of Strings share "str_index"; "str_conv", the conversion over n rows
 * -- or over the store's entries on the dictionary side: two offsets (16 B) per row, on the rows side its index word
 * (8 B) too, 9 B written per row (size: 8 B), and the strings' bytes once each where they are known -- on the
 * dictionary side the whole byte array, for size one byte per slot; on the rows side of the parsers they depend on
 * the data and are not counted; "str_conv_lookup", the dictionary side's row gather: 26 B per row (size: 25 B);
 * size's lengths / scan / compaction are timed as "str_conv_starts", without bytes;
 * toString() / string concatenation share "str_index" too; their distinct-tuple pass runs the hash kernels untimed;
 * "str_make_lengths", one thread per distinct tuple, declares no bytes; "str_make_starts" is the write pass's plan
 * (scan / compaction), without bytes; "str_make", the write pass: the output bytes written once + per distinct tuple
 * two offsets (16 B) per STR operand and 8 B per Long operand; "str_store_merge", the copy into the grown store:
 * the old store's bytes read and written once and the new entries' bytes likewise, its plan (scan / compaction) timed
 * as "str_store_merge_starts", without bytes; "str_make_gather": 8 B read and
 * 9 B written per row;
 * var-length count(DISTINCT b): "reach_level", one level of a batch of 64 W sources: 8 B per pooled pair + 8 W B of
 * frontier words per relationship + the 3 n W 8 B of state (the flat form: the relationship columns instead of the
 * pool, its state counted under "reach_final"); "reach_count_level": 8 B (narrow) or 16 B per relationship;
 * "reach_count_final": 20 B per word of 32 ids; "reach_part", the partition by target slice, declares none;
 * var-length collect(DISTINCT b): "reach_list_count", pass 1 of a batch's extraction: the n W 8 B of hit words read
 * + 4 B per (tile, source) count written; "reach_list_write", pass 2: 8 B per element written + the n W 8 B of hit
 * words + 4 B per (tile, source) base read (the global form: 8 B per element + 12 B per word of 32 ids);
 * "reach_list_starts", the hit words, scans and compaction, declares none;
 * 0 otherwise; then the counter resets. */
capsmi_status capsmi_session_kernel_bytes(capsmi_session* s, const char* name, double* bytes);
/* fused-path routing of lazy plans: enable / disable (default on; off = operator by operator, for
 * A/B checks), and the number of plans routed to fused entry point `name` ("expand", "expand_count",
 * "two_hop", "triangle", "var_length", "var_length_distinct") since the session started */
capsmi_status capsmi_session_set_fused(capsmi_session* s, int32_t enabled);
/* query parameters (the CypherMap handed to asSparkSQLExpr): CAPSMI_X_PARAM `arg` = index into
 * `params`.  A scalar has count 1 (is_list 0); a list has is_list 1 and `count` values.  Values are
 * copied; programs built after the call see them. */
typedef struct {
    int64_t ival;     /* literal payload, as capsmi_expr.ival */
    int32_t is_null;
    int32_t reserved;
} capsmi_value;
typedef struct {
    int32_t type;     /* CAPSMI_I64 / F64 / BOOL / STR (dictionary code) */
    int32_t is_list;
    int32_t count;
    int32_t reserved;
    const capsmi_value* values;
} capsmi_param;
capsmi_status capsmi_session_set_params(capsmi_session* s, int32_t nparams, const capsmi_param* params);
/* The string store: the bytes behind the codes of CAPSMI_STR values, which CAPSMI_X_STARTS_WITH / ENDS_WITH /
 * CONTAINS read.  String i has code codes[i] and the UTF-8 bytes bytes[offsets[i] .. offsets[i+1]); codes are
 * strictly ascending; offsets has nstrings + 1 entries, starts at 0 and never decreases.  The inputs are copied to
 * the device (codes and offsets are kept on the host too); the call replaces the previous store as a whole, and
 * nstrings == 0 clears it.  A program reads the store that is registered when its action runs, so a caller whose
 * codes are stable registers supersets and nodes built earlier stay valid.  Malformed arrays or a null session
 * are CAPSMI_ERR_ILLEGAL_ARGUMENT.  On several ranks each registers its own store (the operators are row-local). */
capsmi_status capsmi_session_set_strings(capsmi_session* s, int64_t nstrings, const int64_t* codes,
                                         const int64_t* offsets, const char* bytes);
/* The string sink: how strings made on the device (CAPSMI_X_TO_STRING, CAPSMI_X_CONCAT) get their codes.  A code
 * comes from a dictionary the caller owns, so the library cannot invent one: an action that has made strings calls
 * `fn` on the thread that runs the action, once per lowered node, with host arrays that hold n >= 1 strings --
 * string i is bytes[offsets[i] .. offsets[i+1]) -- and the sink writes one code per string into codes_out and
 * returns 0.  The strings may repeat (two operand tuples can give equal bytes, "a" + "bc" and "ab" + "c") and may be
 * in the caller's dictionary already.  Equal bytes must get equal codes, distinct bytes distinct codes; keeping code
 * order equal to string order is the caller's business, as it is for capsmi_session_set_strings.  The sink must not
 * call into the session.  After the call the library merges the entries whose codes the registered store does not
 * hold into that store (codes stay strictly ascending; the old bytes move device to device; entries already present
 * are dropped, so a repeated query merges nothing).  CAPSMI_ERR_ILLEGAL_ARGUMENT, with the store left as it was: a
 * non-zero return, two different byte strings with one code, a code the store already holds for different bytes.
 * fn NULL removes the sink.  On several ranks each rank's sink is its own (the operators are row-local). */
typedef int32_t (*capsmi_string_sink_fn)(void* ctx, int64_t n, const int64_t* offsets, const char* bytes,
                                         int64_t* codes_out);
capsmi_status capsmi_session_set_string_sink(capsmi_session* s, capsmi_string_sink_fn fn, void* ctx);
/* entries of the registered string store (0: none is registered) */
capsmi_status capsmi_session_string_count(capsmi_session* s, int64_t* out);
/* route "miss" counts materialisations in which a pattern over entity tables (joins of node and
 * relationship scans) matched no fused shape and ran operator by operator */
capsmi_status capsmi_session_route_count(capsmi_session* s, const char* name, int64_t* count);
/* refuse (CAPSMI_ERR_UNSUPPORTED, before any work) an unrouted join whose estimated output -- System-R
 * row estimates, entity key columns' distinct counts from their scans -- exceeds max_bytes of 8-byte
 * words; 0 (the default) = no limit.  A guard against a pattern that misses every fused shape and
 * would materialise its bindings (~10^13 rows at the C3 scale). */
capsmi_status capsmi_session_set_unrouted_limit(capsmi_session* s, int64_t max_bytes);

/* ---- tables (CypherTable: okapi-api/.../api/table/CypherTable.scala:41-68) -------- */
/* CAPSNodeTable/CAPSRelationshipTable ingest (spark-cypher/.../api/io/CAPSTable.scala:47-214): copies */
capsmi_status capsmi_table_from_host(capsmi_session* s, int32_t ncols, const capsmi_col_desc* cols,
                                     int64_t nrows, capsmi_table** out);
/* same, but `data`/`valid` are device pointers on this session's device (copied, stream-ordered) */
capsmi_status capsmi_table_from_device(capsmi_session* s, int32_t ncols, const capsmi_col_desc* cols,
                                       int64_t nrows, capsmi_table** out);
capsmi_status capsmi_table_retain(capsmi_table* t);
capsmi_status capsmi_table_release(capsmi_table* t);
/* CypherTable.size -> DataFrameTable.size = df.count() (SparkTable.scala:59) */
capsmi_status capsmi_table_size(const capsmi_table* t, int64_t* out);
/* CypherTable.physicalColumns / columnType (SparkTable.scala:51-53) */
capsmi_status capsmi_table_num_columns(const capsmi_table* t, int32_t* out);
capsmi_status capsmi_table_column_name(const capsmi_table* t, int32_t col, char* buf, size_t n);
capsmi_status capsmi_table_column_type(const capsmi_table* t, int32_t col, int32_t* out);
capsmi_status capsmi_table_column_index(const capsmi_table* t, const char* name, int32_t* out);
capsmi_status capsmi_table_column_nullable(const capsmi_table* t, int32_t col, int32_t* out);
/* the whole schema in one call (no materialisation): *ncols columns; names NUL-separated into
 * `names` (names_len bytes), types[i] and nullable[i] for i < min(*ncols, max_cols); ILLEGAL_ARGUMENT
 * if the names do not fit */
capsmi_status capsmi_table_schema(const capsmi_table* t, int32_t* ncols, char* names, size_t names_len, int32_t* types,
                                  int32_t* nullable, int32_t max_cols);
/* CypherTable.rows / CAPSRecords.collect (SparkTable.scala:55-57, CAPSRecords.scala:136-143):
 * copies rows [offset, offset+n) of one column to the host; host_valid may be NULL */
capsmi_status capsmi_table_export(const capsmi_table* t, int32_t col, void* host_data, uint8_t* host_valid,
                                  int64_t offset, int64_t n);
/* rows [offset, offset+n) of a list column (CAPSMI_LIST_*) to the host: row i's elements are
 * host_values[host_offsets[i] .. host_offsets[i+1]) (host_offsets has n + 1 entries; a null row is
 * empty with host_valid[i] = 0; host_valid may be NULL).  *nvalues = the number of elements of the
 * range; host_values == NULL only reports it (host_offsets may then be NULL too); otherwise
 * values_cap must be >= *nvalues, else ILLEGAL_ARGUMENT.  Elements are 8-byte words of the element
 * type.  (CAPSRecords.collect of a CTList column, rowToCypherMap.scala) */
capsmi_status capsmi_table_export_list(const capsmi_table* t, int32_t col, int64_t offset, int64_t n,
                                       int64_t* host_offsets, uint8_t* host_valid, void* host_values,
                                       int64_t values_cap, int64_t* nvalues);
/* List-property ingest, as CAPSNodeTable / CAPSRelationshipTable take array columns of their DataFrame
 * (CAPSTable.scala:47-214): `t` (materialised by the call) plus a list column `name` of type CAPSMI_LIST +
 * elem_type built from host CSR arrays.  Row i's elements are host_values[host_offsets[i] .. host_offsets[i+1]):
 * 8-byte words of the element type, no element nulls (as in Collect's stores).  host_offsets has nrows + 1
 * int64 entries, non-decreasing, starting at 0; its last entry is the value count.  host_valid (nrows bytes,
 * 1 = non-null list) may be NULL.  Malformed offsets, a bad element type or an existing column `name` are
 * CAPSMI_ERR_ILLEGAL_ARGUMENT.  Copies; the result is a plain table (no entity registration). */
capsmi_status capsmi_table_add_list_column(capsmi_table* t, const char* name, int32_t elem_type,
                                           const int64_t* host_offsets, const void* host_values,
                                           const uint8_t* host_valid, capsmi_table** out);
/* zero-copy device view of a column (valid pointer NULL when the column has no nulls) */
capsmi_status capsmi_table_column_device_ptr(const capsmi_table* t, int32_t col, const void** data,
                                             const uint8_t** valid);

/* ---- entity tables (the input contract) ------------------------------------------------
 * CAPSNodeTable / CAPSRelationshipTable construction with EntityTable.verify
 * (okapi-relational/.../api/io/EntityTable.scala:59-65, 105-131, 155-164): the id keys must be
 * non-nullable Long columns ("id key", "start node", "end node"), optional-label and relationship-type
 * flag columns non-nullable Boolean, and the columns in canonical order
 *   node: [id, label flags..., properties sorted by name]
 *   rel:  [id, source, target, type flags..., properties sorted by name]     (EntityMapping.scala:50)
 * else CAPSMI_ERR_ILLEGAL_ARGUMENT.  The result shares the input's columns and is what the fused-path
 * recogniser (below) treats as a scanned entity table; registration records the id range.
 * capsmi_rel_table also keeps, with the result's endpoint columns, a 32-bit copy of each (the value minus the
 * smallest endpoint) when the table has rows and its endpoints span at most 2^32 ids: one pass over both
 * columns at registration and 8 bytes of device memory per relationship, shared by every table derived from
 * the result (select, rename, skip, limit, cache).  The partitioned 2-hop and var-length entry points read the
 * copies in their first pass instead of the Long columns; results are the same.  CAPSMI_NARROW=off at
 * registration keeps none; off at a query reads none.  Route counts (capsmi_session_route_count):
 * "narrow_built" per table that got copies, "pass1_narrow" per first-pass launch that read them.
 * capsmi_rel_table likewise keeps endpoint presence words when the table has rows and its endpoints span at most
 * 2^26 ids: four bitmaps over the endpoints' window (ids that are the target / the source of a relationship that
 * is no self-loop, ids with at least one / two self-loops).  They cost two runs of the partition's first pass and
 * first hop at registration (about 8 ms for 2^30 relationships on MI355X, with a transient pool of 8 bytes per
 * relationship) and 4 bits of device memory per id of the window, and are shared like the copies.  The first hop
 * of a 2-hop whose first node is unfiltered over the query's id domain is answered from them without reading the
 * relationships, when every table of the walk offers words for exactly the rows it is walked with (a view behind
 * a later skip or limit, or with a replaced endpoint column, offers none) and the tables' windows lie inside the
 * domain; results are the same.  A registration of endpoint columns that already carry words valid for each other
 * reuses them.  CAPSMI_PRESENCE=off at registration keeps none; off at a query reads none.  Route counts:
 * "presence_built" / "presence_reused" per registration, "hop1_presence" per first hop answered from words. */
capsmi_status capsmi_node_table(capsmi_table* t, const char* id_col, int32_t nlabels, const char* const* label_cols,
                                capsmi_table** out);
capsmi_status capsmi_rel_table(capsmi_table* t, const char* id_col, const char* src_col, const char* dst_col,
                               int32_t ntypes, const char* const* type_cols, capsmi_table** out);
/* Graph-level id compaction (the analogue of caching a graph at creation, CAPSGraphFactory.create /
 * CachedDataSource): numbers every node id of `nodes` and every endpoint of `rels` densely and keeps
 * the dense columns with the tables, so graphs whose Long ids are sparse, large or carry tag bits
 * (Tags.scala:36-55) reach the fused kernels.  Results keep the original ids. */
capsmi_status capsmi_graph_compact(capsmi_session* s, int32_t nnodes, capsmi_table* const* nodes, int32_t nrels,
                                   capsmi_table* const* rels, int64_t* dense_ids);
/* kind 0 = plain table, 1 = node table, 2 = relationship table; [*id_lo, *id_hi) = range of the ids
 * (node) or of both endpoints (relationship) */
capsmi_status capsmi_table_entity(const capsmi_table* t, int32_t* kind, int64_t* id_lo, int64_t* id_hi);
/* CAPSRelationshipTable.fromMapping's relationship-type flattening (spark-cypher/.../api/io/CAPSTable.scala:189-204):
 * the String column `type_col` (dictionary codes) becomes one non-nullable Boolean column per type,
 * out_cols[i] = (type_col = type_codes[i]), and type_col is dropped. */
capsmi_status capsmi_flatten_rel_types(capsmi_table* t, const char* type_col, int32_t ntypes, const int64_t* type_codes,
                                       const char* const* out_cols, capsmi_table** out);

/* ---- Table[T] operators -------------------------------------------------------------
 * Operators are lazy, like DataFrameTable's Spark plans: each returns a table whose schema is known
 * at once (name / type / nullability queries, errors for unknown columns or bad programs) and whose
 * rows are computed when first needed -- capsmi_table_size, _export, _column_device_ptr,
 * _fingerprint, or a graph entry point consuming it (RelationalCypherRecords.size -> df.count(),
 * SparkTable.scala:59).  At that point the plan is matched against the fused graph kernels: joins of
 * registered node / relationship tables in the Expand / ExpandInto / BoundedVarLengthExpand shapes
 * RelationalPlanner emits (RelationalPlanner.scala:113-177, VarLengthExpandPlanner.scala:46-310),
 * their uniqueness and node filters, and the aggregate or projection on top run as one fused call;
 * anything else runs operator by operator.  A materialised table keeps its rows (shared sub-plans
 * run once: the Cache analogue). */
capsmi_status capsmi_cache(capsmi_table* t, capsmi_table** out);                         /* Table.scala:52  */
capsmi_status capsmi_select(capsmi_table* t, int32_t ncols, const char* const* cols,
                            capsmi_table** out);                                        /* Table.scala:60  */
capsmi_status capsmi_filter(capsmi_table* t, int32_t nnodes, const capsmi_expr* prog,
                            capsmi_table** out);                                        /* Table.scala:70  */
capsmi_status capsmi_drop(capsmi_table* t, int32_t ncols, const char* const* cols,
                          capsmi_table** out);                                          /* Table.scala:78  */
capsmi_status capsmi_join(capsmi_table* l, capsmi_table* r, int32_t join_type, int32_t npairs,
                          const char* const* lcols, const char* const* rcols,
                          capsmi_table** out);                                          /* Table.scala:88  */
capsmi_status capsmi_union_all(capsmi_table* a, capsmi_table* b, capsmi_table** out);   /* Table.scala:96  */
capsmi_status capsmi_order_by(capsmi_table* t, int32_t nkeys, const char* const* cols,
                              const int32_t* descending, capsmi_table** out);           /* Table.scala:104 */
capsmi_status capsmi_skip(capsmi_table* t, int64_t n, capsmi_table** out);              /* Table.scala:112 */
capsmi_status capsmi_limit(capsmi_table* t, int64_t n, capsmi_table** out);             /* Table.scala:120 */
capsmi_status capsmi_distinct(capsmi_table* t, capsmi_table** out);                     /* Table.scala:127 */
capsmi_status capsmi_distinct_on(capsmi_table* t, int32_t ncols, const char* const* cols,
                                 capsmi_table** out);                                   /* SparkTable.scala:234-235 */
capsmi_status capsmi_group(capsmi_table* t, int32_t nby, const char* const* by, int32_t naggs,
                           const capsmi_agg* aggs, capsmi_table** out);                 /* Table.scala:147 */
capsmi_status capsmi_with_columns(capsmi_table* t, int32_t ncols, const capsmi_expr_column* cols,
                                  capsmi_table** out);                                  /* Table.scala:159 */
capsmi_status capsmi_with_column_renamed(capsmi_table* t, const char* old_name, const char* new_name,
                                         capsmi_table** out);                           /* Table.scala:168 */
/* UNWIND.  RelationalPlanner lowers logical.Unwind(list, item, in) to in.add(Explode(list) as item)
 * (RelationalPlanner.scala:94-96), i.e. Table.withColumns (Table.scala:159) of an Explode expression, which
 * SparkSQLExprMapper maps to functions.explode (SparkSQLExprMapper.scala:237-241).  Row i of `t`, whose list in
 * the CAPSMI_LIST_* column `list_col` has L_i elements, becomes L_i output rows; a null or an empty list yields
 * no row (explode, not explode_outer).  The result holds every input column, `list_col` included (withColumn
 * keeps it), and a non-nullable column `item_name` of the element type, which replaces a column of that name if
 * there is one and is appended otherwise (the capsmi_with_columns rule).  Output rows are ordered by (input row,
 * element position).  A `list_col` that is no list column is CAPSMI_ERR_ILLEGAL_ARGUMENT.  Lazy like every
 * operator: a filter that reads the item stays above the explode, filters on other columns run below it, and
 * only the payload columns that something above reads are gathered; the node matches no fused shape, and the
 * plan under it is routed as usual.  Row-local: the result of a partitioned table is partitioned, and no
 * collective is called. */
capsmi_status capsmi_explode(capsmi_table* t, const char* list_col, const char* item_name, capsmi_table** out);
/* The same for a list that is not a column: explode(array(lit...)) of a ListLit or a list Param
 * (SparkSQLExprMapper.scala:86-89, 111-112, 237-241).  Every input row is repeated `count` times, with
 * item = values[j] (ival as capsmi_expr.ival, of type elem_type = CAPSMI_I64 ... CAPSMI_STR) in its j-th copy;
 * order (input row, j).  The item column is nullable exactly when some value has is_null set.  count == 0
 * gives zero rows.  Values are copied. */
capsmi_status capsmi_explode_values(capsmi_table* t, int32_t elem_type, int32_t count, const capsmi_value* values,
                                    const char* item_name, capsmi_table** out);

/* range(from, to[, step]) as a list column (Range, SparkSQLExprMapper.scala:243-245; the reference's rangeUdf,
 * CAPSFunctions.scala:50, Scala's from.to(to, step), over Long).  The three programs are scalar Long
 * expressions over `t` (step_prog NULL with step_nnodes 0: the literal 1); the result is `t` plus a
 * CAPSMI_LIST_I64 column `name` under the capsmi_with_columns replace-or-append rule.  Row i's list is from,
 * from + step, ... up to the last element <= to (step > 0) or >= to (step < 0); empty when `to` lies on the
 * wrong side of `from`; NULL when an operand is NULL.  Lengths are computed without signed overflow and no
 * element past `to` is ever formed, so operands at the ends of the Long range are safe.  A non-Long operand is
 * CAPSMI_ERR_ILLEGAL_ARGUMENT when the node is built; a row with step == 0 fails the action with
 * CAPSMI_ERR_ILLEGAL_ARGUMENT ("range: step 0"), as Scala throws; a total element count beyond what the
 * session can allocate is CAPSMI_ERR_UNSUPPORTED with the count in the message, decided from the scanned
 * lengths before anything sized by the count is allocated.  "Can allocate" is judged against the device's
 * whole memory (8 bytes per element), and a single row of 2^40 elements or more (of 2^62 / rows elements where that is less, so that the sum
 * cannot overflow) is always refused (its length
 * is not counted further: the message then says "N or more"); a count that the device could hold but that
 * is not free at the moment, the per-row buffers included, is the allocator's CAPSMI_ERR_OUT_OF_MEMORY.
 * Lazy and row-local: no collective is called and a partitioned table stays partitioned. */
capsmi_status capsmi_with_range_column(capsmi_table* t, int32_t from_nnodes, const capsmi_expr* from_prog,
                                       int32_t to_nnodes, const capsmi_expr* to_prog, int32_t step_nnodes,
                                       const capsmi_expr* step_prog, const char* name, capsmi_table** out);

/* labels(n) and keys(n) as a list column (Labels / Keys, SparkSQLExprMapper.scala:192-208; the reference's
 * get_node_labels / get_property_keys UDFs over array(flag or property columns), CAPSFunctions.scala:73-91).
 * The result is `t` plus a non-nullable CAPSMI_LIST_STR column `name` under the capsmi_with_columns
 * replace-or-append rule (`name` may equal one of `cols`).  Row r's list holds elem_codes[i] (dictionary codes)
 * for every i, in the order given, whose column cols[i] passes in row r:
 *   CAPSMI_MASK_TRUE      every column is CAPSMI_BOOL (anything else: CAPSMI_ERR_ILLEGAL_ARGUMENT when the node
 *                         is built); a column passes where it is non-null and TRUE.  A NULL flag is not set, and
 *                         a TRUE word stored under a null row is not seen.
 *   CAPSMI_MASK_NOT_NULL  columns of any type, list columns included; a column passes where the row is
 *                         non-null.  Only validity is read: a non-nullable column always passes.
 * The list is never NULL: filterWithMask's `case (label, true)` and filterNotNull's `value != null`
 * (CAPSFunctions.scala:73-91) skip the null elements of the array the UDF receives, so a null entity (an
 * OPTIONAL MATCH miss) yields [].  This is a reading of the reference's source, not an observation of a run.
 * The library does not sort: the caller passes the names in the reference's order (sortBy(_._1) for labels,
 * :198; sortBy(_.key.name) for keys, :205).  ncols == 0 is legal (every row gets []; the reference's array()
 * for a graph without labels); ncols > 64 is CAPSMI_ERR_UNSUPPORTED when the node is built (one 64-bit mask
 * word per row).  The element count is checked as capsmi_with_range_column checks it, before anything sized by
 * it is allocated (it is at most 64 per row, so only memory pressure can trigger it).
 * Lazy and row-local: no collective is called and a partitioned table stays partitioned. */
enum { CAPSMI_MASK_TRUE = 0, CAPSMI_MASK_NOT_NULL = 1 };
capsmi_status capsmi_with_mask_list_column(capsmi_table* t, int32_t mode, int32_t ncols, const char* const* cols,
                                           const int64_t* elem_codes, const char* name, capsmi_table** out);

/* ---- graph fast path ------------------------------------------------------------------
 * The relational planner lowers Expand into `join(relScan, source = start)` then
 * `join(nodeScan, end = target)` (RelationalPlanner.scala:113-137).  When the shim sees that
 * shape over base entity tables with dense Long ids it calls these fused entry points
 * instead; results are identical row multisets.
 *
 * A capsmi_bitmap is a node scan + label/property predicate (ScanGraph.scanOperator,
 * ScanGraph.scala:61-96, plus Filter) collapsed to one bit per id in [id_lo, id_hi). */
capsmi_status capsmi_bitmap_create(capsmi_session* s, int64_t id_lo, int64_t id_hi, capsmi_bitmap** out);
/* OR in the ids of node-table rows whose predicate is TRUE (nnodes = 0: every row).
 * Ids outside [id_lo, id_hi) or null ids are an ILLEGAL_ARGUMENT error. */
capsmi_status capsmi_bitmap_add_scan(capsmi_bitmap* b, capsmi_table* nodes, const char* id_col,
                                     int32_t nnodes, const capsmi_expr* pred);
/* number of set bits, and whether every scanned row contributed a distinct id (no id in two
 * scanned rows: the fused paths require it, since CAPS would emit one row per table occurrence,
 * ScanGraph.scala:72-76) */
capsmi_status capsmi_bitmap_stats(capsmi_bitmap* b, int64_t* set_bits, int32_t* unique_rows);
capsmi_status capsmi_bitmap_release(capsmi_bitmap* b);
/* the bitmap's device words (uint32, bit i of word w <-> id lo + 32w + i) for collectives: a rank
 * scans its owned node rows, the ranks all-gather their owned word slices into these words, then
 * capsmi_bitmap_refresh re-derives the set-bit count (synchronises); `unique_rows` states whether
 * every rank's scan was duplicate-free (the all-reduced AND of capsmi_bitmap_stats) */
capsmi_status capsmi_bitmap_words(capsmi_bitmap* b, uint32_t** words, int64_t* nwords);
capsmi_status capsmi_bitmap_refresh(capsmi_bitmap* b, int32_t unique_rows);
/* the same without the device popcount (no synchronisation): the caller states the set-bit count,
 * e.g. the all-reduced sum of every rank's capsmi_bitmap_stats over its owned rows, taken before
 * the all-gather */
capsmi_status capsmi_bitmap_assume(capsmi_bitmap* b, int64_t set_bits, int32_t unique_rows);
/* stream-ordered device copy of words [w_begin, w_end): to_bitmap = 0 copies bitmap -> ext,
 * 1 copies ext -> bitmap (ext: a caller device buffer of w_end - w_begin words).  Like every call
 * taking a caller device pointer, the copy is queued on the SESSION's stream: `ext` must already be
 * written (allocated, zero-filled, ...) in that stream's order -- run the host's own device work on
 * the same stream (capsmi_session_use_stream) or make the session stream wait on it -- and the host
 * may read it only after capsmi_session_sync or stream-ordered work behind it */
capsmi_status capsmi_bitmap_copy_words(capsmi_bitmap* b, int64_t w_begin, int64_t w_end, uint32_t* ext,
                                       int32_t to_bitmap);

/* 1-hop Expand + node filters, fused (C2):
 *   MATCH (a)-[r]->(b) WHERE src_ok(a) AND dst_ok(b)
 * = rels ⋈ a-scan ⋈ b-scan; returns the rel rows that survive, projected on `out_cols`
 * (renamed to `out_names`, or kept when out_names == NULL). */
capsmi_status capsmi_expand_filter(capsmi_session* s, capsmi_table* rels, const char* src_col,
                                   const char* dst_col, const capsmi_bitmap* src_ok,
                                   const capsmi_bitmap* dst_ok, int32_t nout, const char* const* out_cols,
                                   const char* const* out_names, capsmi_table** out);

/* 2-hop with relationship uniqueness (C3), fused, never materialising the bindings:
 *   MATCH (a)-[r1]->(b)-[r2]->(c) WHERE a_ok(a) AND b_ok(b) AND c_ok(c)   [r1 <> r2 implied]
 *   RETURN count(DISTINCT c)
 * `rels` is one or more relationship tables of the scanned type (their union is the rel scan). */
capsmi_status capsmi_two_hop_count_distinct(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                            const char* src_col, const char* dst_col,
                                            const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok,
                                            const capsmi_bitmap* c_ok, int64_t* out_distinct);
/* count(*) of the same MATCH, closed form: sum_b [b_ok] inA(b) * outC(b) - #eligible self-loops */
capsmi_status capsmi_two_hop_count(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                   const char* src_col, const char* dst_col, const capsmi_bitmap* a_ok,
                                   const capsmi_bitmap* b_ok, const capsmi_bitmap* c_ok, int64_t* out_rows);

/* Phased form of capsmi_two_hop_count_distinct for the multi-GPU path.  The caller
 * owns the exchange (RCCL all-gather of the owned bitmap slice between the two phases).
 * Bitmaps are uint32 words, bit i of word w <-> id lo+32w+i; mid_words span b_ok's id range and
 * dst_words c_ok's.
 * mid_words:  2 x nwords (X1 then X2), zeroed by the call.  X1(b): b can be the middle of a 2-hop
 *             whose second edge is not a self-loop; X2(b): ... whose second edge is a self-loop at b.
 * dst_words:  nwords, zeroed by the call; marks every reachable c.  `scratch_words`: nwords. */
capsmi_status capsmi_two_hop_mark_mid(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                      const char* src_col, const char* dst_col, const capsmi_bitmap* a_ok,
                                      const capsmi_bitmap* b_ok, uint32_t* mid_words, uint32_t* scratch_words);
capsmi_status capsmi_two_hop_mark_dst(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                      const char* src_col, const char* dst_col, const capsmi_bitmap* b_ok,
                                      const capsmi_bitmap* c_ok, const uint32_t* mid_words, uint32_t* dst_words);
/* Radix-partitioned relationship layout for the 2-hop kernels: rows of the union of `rels` with both
 * endpoints in [id_lo, id_hi) (hi - lo <= 2^30), packed to 32-bit ids and grouped by 2-D cell
 * (target slice of 2^19 ids) x (source slice).  Building it is part of the cold query; keeping it
 * across queries is the Cache analogue (DataFrameTable.cache, SparkTable.scala:240-246). */
typedef struct capsmi_relpart capsmi_relpart;
capsmi_status capsmi_relpart_build(capsmi_session* s, int32_t nrels, capsmi_table* const* rels, const char* src_col,
                                   const char* dst_col, int64_t id_lo, int64_t id_hi, capsmi_relpart** out);
capsmi_status capsmi_relpart_size(const capsmi_relpart* p, int64_t* kept_rows);
capsmi_status capsmi_relpart_release(capsmi_relpart* p);
/* Layout check (test support, synchronous): per 2-D cell c (target slice major) the number of pairs and
   the wrapping sum of mix64((source - lo) << 32 | (target - lo)) over them; pairs stored outside their
   own cell are counted in *misplaced.  counts/sums hold *ncells entries each; pass NULL arrays to read
   the cell geometry only (*ncells, *ns = source slices per target slice, *sbits, *tbits). */
capsmi_status capsmi_relpart_digest(const capsmi_relpart* p, int64_t* ncells, int64_t* ns, int32_t* sbits,
                                    int32_t* tbits, int64_t* counts, uint64_t* sums, int64_t* misplaced);
/* capsmi_relpart_build followed by capsmi_two_hop_mark_mid_part, with hop 1 run by the build's second
 * pass when a_ok covers the whole id domain (the cold 2-hop: one pass fewer over the relationships) */
capsmi_status capsmi_relpart_build_mark_mid(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                            const char* src_col, const char* dst_col, const capsmi_bitmap* a_ok,
                                            const capsmi_bitmap* b_ok, uint32_t* mid_words, uint32_t* scratch_words,
                                            capsmi_relpart** out);
/* the phased 2-hop over a partitioned layout (same contract as capsmi_two_hop_mark_mid/_dst) */
capsmi_status capsmi_two_hop_mark_mid_part(capsmi_session* s, const capsmi_relpart* p, const capsmi_bitmap* a_ok,
                                           const capsmi_bitmap* b_ok, uint32_t* mid_words, uint32_t* scratch_words);
capsmi_status capsmi_two_hop_mark_dst_part(capsmi_session* s, const capsmi_relpart* p, const capsmi_bitmap* b_ok,
                                           const capsmi_bitmap* c_ok, const uint32_t* mid_words, uint32_t* dst_words);
/* whole query over a cached layout */
capsmi_status capsmi_two_hop_count_distinct_part(capsmi_session* s, const capsmi_relpart* p, const capsmi_bitmap* a_ok,
                                                 const capsmi_bitmap* b_ok, const capsmi_bitmap* c_ok,
                                                 int64_t* out_distinct);
/* Undirected Expand patterns, fused.  An undirected Expand is the union of the outgoing branch and the
 * incoming branch over relationships whose start differs from their end (RelationalPlanner.scala:126-136):
 *   hops = 1: MATCH (a)-[r]-(b) WHERE a_ok(a) AND b_ok(b)
 *   hops = 2: MATCH (a)-[r1]-(b)-[r2]-(c) WHERE a_ok(a) AND b_ok(b) AND c_ok(c)   [r1 <> r2 implied]
 * RETURN count(*) (kind 0), count(DISTINCT the last node) (kind 1) or count(DISTINCT a) (kind 2); c_ok
 * is ignored for one hop.  The bitmaps share one id domain. */
capsmi_status capsmi_undirected_count(capsmi_session* s, int32_t nrels, capsmi_table* const* rels, const char* src_col,
                                      const char* dst_col, int32_t hops, const capsmi_bitmap* a_ok,
                                      const capsmi_bitmap* b_ok, const capsmi_bitmap* c_ok, int32_t kind, int64_t* out);
/* BoundedVarLengthExpand + grouped count, fused (C5):
 *   MATCH (a)-[r*lower..upper]->(b) WHERE a_ok(a) AND b_ok(b) RETURN id(a) AS <id_name>, count(*) AS <count_name>
 * with edge-distinct paths (VarLengthExpandPlanner.scala:83-136, 179-180), 0 <= lower <= upper <= 4,
 * upper >= 1 (upper 4: ids below 2^24 - 1).  lower = 0 adds the zero-length path of every a_ok node (copyEntity, :146-153, 190-210:
 * b is a copy of a, without b's node scan).  One output row per a with at least one path.  a_ok and
 * b_ok must share one id domain. */
capsmi_status capsmi_var_length_count(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                      const char* src_col, const char* dst_col, const capsmi_bitmap* a_ok,
                                      const capsmi_bitmap* b_ok, int32_t lower, int32_t upper, const char* id_name,
                                      const char* count_name, capsmi_table** out);
/* BoundedVarLengthExpand + count(DISTINCT b), fused: k-hop reach by bit-parallel BFS (k_reach.hip).
 *   MATCH (a)-[r*lower..upper]->(b) WHERE a_ok(a) AND b_ok(b)
 *   RETURN id(a) AS <id_name>, count(DISTINCT b) AS <count_name>
 * lower 0 or 1, any upper >= 1 (a level budget: a frontier dies after at most n levels).
 * Lemma: for lower <= 1, b ends a relationship-distinct path of length in [1, upper] from a iff b ends a walk of
 * that length -- cutting the stretch between two uses of a repeated relationship leaves a shorter walk from a to b
 * that keeps one relationship -- so the distinct ends are plain bounded reachability.
 * lower >= 2 is CAPSMI_ERR_NOT_IMPLEMENTED (the lemma fails there: use the join plan).
 * lower = 0 adds the zero-length path of every a_ok node (copyEntity, VarLengthExpandPlanner.scala:146-153,
 * 190-210: b is a copy of a, without b's node scan), so a counts itself whatever b_ok(a) says, and once only when
 * a cycle also returns to it.  Relationships with an endpoint outside the bitmaps' id domain are ignored.  One
 * output row per a with a non-empty set, in no particular order.  a_ok and b_ok must share one id domain. */
capsmi_status capsmi_var_length_count_distinct(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                               const char* src_col, const char* dst_col, const capsmi_bitmap* a_ok,
                                               const capsmi_bitmap* b_ok, int32_t lower, int32_t upper,
                                               const char* id_name, const char* count_name, capsmi_table** out);
/* The ungrouped form: MATCH (a)-[r*lower..upper]->(b) WHERE a_ok(a) AND b_ok(b) RETURN count(DISTINCT b), the size
 * of the union of the per-a sets above: one BFS from all of a_ok.  The same lemma (walks and relationship-distinct
 * paths of length in [1, upper] end at the same nodes for lower <= 1; lower >= 2 is CAPSMI_ERR_NOT_IMPLEMENTED)
 * and the same lower = 0 rule: every a_ok node counts, whatever b_ok says of it, once. */
capsmi_status capsmi_var_length_reach_count(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                            const char* src_col, const char* dst_col, const capsmi_bitmap* a_ok,
                                            const capsmi_bitmap* b_ok, int32_t lower, int32_t upper,
                                            int64_t* out_distinct);
/* BoundedVarLengthExpand + collect(DISTINCT b), fused: the sets that capsmi_var_length_count_distinct counts, as lists,
 * read off the same bit-parallel BFS (k_reach.hip).
 *   MATCH (a)-[r*lower..upper]->(b) WHERE a_ok(a) AND b_ok(b)
 *   RETURN id(a) AS <id_name>, collect(DISTINCT b) AS <list_name> [, count(DISTINCT b) AS <count_name>]
 * The same lemma (for lower <= 1 the ends of the relationship-distinct paths are the ends of the walks of length in
 * [1, upper]: DESIGN.md section 4), so lower >= 2 is CAPSMI_ERR_NOT_IMPLEMENTED (use the join plan), and the same
 * lower = 0 rule: a's list holds a itself whatever b_ok(a) says, once, also when a cycle returns to it.  The list
 * column is CAPSMI_LIST_I64 and is sort_array(collect_set(id(b))) (SparkTable.scala:169-177): the absolute ids,
 * strictly ascending, no duplicates, no nulls.  One row per a with a non-empty list, in no particular order.
 * count_name may be NULL; otherwise the table also carries count(DISTINCT b), which the walk has anyway.
 * Guard: the lists may hold up to |a_ok| n elements; beyond CAPSMI_REACH_LIST_LIMIT (elements, or auto = device
 * memory / 16 B) the call is CAPSMI_ERR_UNSUPPORTED, raised before the batch that crosses the limit is written; the
 * session stays usable.  a_ok and b_ok must share one id domain (fewer than 2^32 ids). */
capsmi_status capsmi_var_length_collect_distinct(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                                 const char* src_col, const char* dst_col, const capsmi_bitmap* a_ok,
                                                 const capsmi_bitmap* b_ok, int32_t lower, int32_t upper,
                                                 const char* id_name, const char* list_name, const char* count_name,
                                                 capsmi_table** out);
/* The ungrouped form: MATCH (a)-[r*lower..upper]->(b) WHERE a_ok(a) AND b_ok(b) RETURN collect(DISTINCT b) AS
 * <list_name>: exactly one row holding the union of the per-a lists above, strictly ascending absolute ids in a
 * CAPSMI_LIST_I64 column, the empty list when nothing is reached (collect_set over no rows).  One BFS from all of
 * a_ok; the same lemma (lower >= 2 is CAPSMI_ERR_NOT_IMPLEMENTED: use the join plan), the same lower = 0 rule (every
 * a_ok node is in the list, whatever b_ok says of it, once) and the same CAPSMI_REACH_LIST_LIMIT guard. */
capsmi_status capsmi_var_length_reach_list(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                           const char* src_col, const char* dst_col, const capsmi_bitmap* a_ok,
                                           const capsmi_bitmap* b_ok, int32_t lower, int32_t upper, const char* list_name,
                                           capsmi_table** out);
/* capsmi_var_length_collect_distinct over remapped ids: the bitmaps and the relationship columns hold dense ids (the
 * domain [a_ok->lo, a_ok->hi) of n ids, as capsmi_graph_compact numbers a graph), and `orig`, a device array of
 * orig_len = n int64, gives the original id of dense id a_ok->lo + d at orig[d].
 *   RETURN id(a) AS <id_name>, collect(DISTINCT b) AS <list_name> [, count(DISTINCT b) AS <count_name>]
 * with id(a) and the list elements in ORIGINAL ids: every list is sort_array(collect_set(id(b))), strictly ascending
 * by signed value (Long order: negative ids first), whatever order orig has.  No list element is sorted: the n
 * original ids are sorted once per call (ORDER BY's radix sort), and the walk of capsmi_var_length_collect_distinct
 * runs over the domain in that order.  The same lemma (for lower <= 1 the ends of the relationship-distinct paths are
 * the ends of the walks of length in [1, upper]: DESIGN.md section 4), so lower >= 2 is CAPSMI_ERR_NOT_IMPLEMENTED
 * (use the join plan); the same lower = 0 rule (a's list holds a itself whatever b_ok(a) says, once); the same
 * CAPSMI_REACH_LIST_LIMIT guard (CAPSMI_ERR_UNSUPPORTED, the session stays usable).  One row per a with a non-empty
 * list, in no particular order; with orig[d] = a_ok->lo + d the table equals capsmi_var_length_collect_distinct's.
 * orig must hold distinct ids: orig_len != n, or an id that occurs twice (seen in the sorted ids, one pass and an
 * 8-byte read-back), is CAPSMI_ERR_ILLEGAL_ARGUMENT.  The call reads orig on the session's stream and keeps no
 * reference to it.  The planner's route on a compacted graph keeps the order with the graph instead of sorting per
 * call. */
capsmi_status capsmi_var_length_collect_distinct_mapped(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                                        const char* src_col, const char* dst_col,
                                                        const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok,
                                                        int32_t lower, int32_t upper, const int64_t* orig,
                                                        int64_t orig_len, const char* id_name, const char* list_name,
                                                        const char* count_name, capsmi_table** out);
/* The ungrouped form over remapped ids: RETURN collect(DISTINCT b) AS <list_name>, exactly one row holding the union
 * of the per-a lists above in ORIGINAL ids, strictly ascending by signed value (Long order), the empty list when
 * nothing is reached.  One BFS from all of a_ok on the dense ids; the answer's bitmap is permuted into the order of
 * the original ids before it is written out.  The same lemma (lower >= 2 is CAPSMI_ERR_NOT_IMPLEMENTED: use the join
 * plan), the same lower = 0 rule, the same CAPSMI_REACH_LIST_LIMIT guard, and the same contract for orig (orig_len
 * ids, distinct, else CAPSMI_ERR_ILLEGAL_ARGUMENT). */
capsmi_status capsmi_var_length_reach_list_mapped(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                                  const char* src_col, const char* dst_col, const capsmi_bitmap* a_ok,
                                                  const capsmi_bitmap* b_ok, int32_t lower, int32_t upper,
                                                  const int64_t* orig, int64_t orig_len, const char* list_name,
                                                  capsmi_table** out);
/* Sharded form of capsmi_var_length_count for one rank of a multi-GPU run.  The
 * rank owns the source ids [own_lo, own_hi); `out_rels` hold the relationships whose source it
 * owns, `in_rels` those from other ranks' sources into its owned ids.  `od` and `y` are caller
 * device buffers of (b_ok->hi - b_ok->lo) int64 each:
 *   begin  writes the rank's partial out-degrees into od -> the caller sums od over ranks in place;
 *   mid    writes the rank's partial Y into y            -> the caller sums y over ranks in place;
 *   finish returns the (id, count) rows of the owned ids.  od / y must stay valid until finish. */
typedef struct capsmi_varlen_shard capsmi_varlen_shard;
capsmi_status capsmi_varlen_shard_begin(capsmi_session* s, int32_t nout, capsmi_table* const* out_rels, int32_t nin,
                                        capsmi_table* const* in_rels, const char* src_col, const char* dst_col,
                                        const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok, int32_t lower,
                                        int32_t upper, int64_t own_lo, int64_t own_hi, int64_t* od,
                                        capsmi_varlen_shard** out);
capsmi_status capsmi_varlen_shard_mid(capsmi_varlen_shard* v, int64_t* y);
capsmi_status capsmi_varlen_shard_finish(capsmi_varlen_shard* v, const char* id_name, const char* count_name,
                                         capsmi_table** out);
capsmi_status capsmi_varlen_shard_release(capsmi_varlen_shard* v);
/* Cyclic triangle count (C4), fused:
 *   MATCH (a)-[r1]->(b)-[r2]->(c)-[r3]->(a) WHERE n_ok(a) AND n_ok(b) AND n_ok(c) RETURN count(*)
 * (two Expands + ExpandInto on (c, a), RelationalPlanner.scala:113-154, plus pairwise uniqueness).
 * The oriented simple graph with multiplicities (a trigraph) is built once; counting can be split into
 * `nparts` interleaved shares of its centers (multi-GPU replicas: each rank counts its part, results sum). */
typedef struct capsmi_trigraph capsmi_trigraph;
capsmi_status capsmi_trigraph_build(capsmi_session* s, int32_t nrels, capsmi_table* const* rels, const char* src_col,
                                    const char* dst_col, const capsmi_bitmap* n_ok, capsmi_trigraph** out);
capsmi_status capsmi_trigraph_count(capsmi_session* s, const capsmi_trigraph* g, int32_t part, int32_t nparts,
                                    int64_t* out_rows);
/* id-domain size and number of oriented (simple, both directions folded) edges of a trigraph */
capsmi_status capsmi_trigraph_stats(const capsmi_trigraph* g, int64_t* nodes, int64_t* oriented_edges);
capsmi_status capsmi_trigraph_release(capsmi_trigraph* g);
capsmi_status capsmi_triangle_count(capsmi_session* s, int32_t nrels, capsmi_table* const* rels, const char* src_col,
                                    const char* dst_col, const capsmi_bitmap* n_ok, int64_t* out_rows);
/* The same pattern grouped by its start: ... RETURN id(a), count(*) -- the bindings per start node (equally the
 * counts per b or per c: the pattern is symmetric under rotation).  `*out` gets two non-nullable Long columns,
 * the graph's own ids (`id_name`) and the counts (`count_name`), one row per node with a non-zero count, in
 * no particular order.  Single device: a trigraph of a distributed build gives CAPSMI_ERR_UNSUPPORTED. */
capsmi_status capsmi_trigraph_count_by_node(capsmi_session* s, const capsmi_trigraph* g, const char* id_name,
                                            const char* count_name, capsmi_table** out);
capsmi_status capsmi_triangle_count_by_node(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                            const char* src_col, const char* dst_col, const capsmi_bitmap* n_ok,
                                            const char* id_name, const char* count_name, capsmi_table** out);
/* The transitive ("feed-forward") triangle over the same trigraph:
 *   MATCH (a)-[r1]->(b)-[r2]->(c)<-[r3]-(a) WHERE n_ok(a) AND n_ok(b) AND n_ok(c) RETURN count(*)
 *   ... RETURN id(a), count(*)     (or id(b), or id(c))
 * Bindings are rows: r1, r2, r3 are pairwise distinct, node variables may coincide, and the one node filter
 * applies to all three positions.  With m(x,y) the multiplicity of x->y for x != y, s(x) the self-loops at x and
 * M(y,z) = m(y,z) + m(z,y), the bindings split by how many of a, b, c coincide:
 *   three distinct nodes   m(a,b) m(b,c) m(a,c); of a simple triangle {x,y,z}, node x receives
 *                            as source a   m(x,y) m(x,z) M(y,z)
 *                            as sink c     m(y,x) m(z,x) M(y,z)
 *                            as middle b   m(y,x) m(x,z) m(y,z) + m(z,x) m(x,y) m(z,y)
 *   a = b = x, c = y != x  s(x) m(x,y) (m(x,y)-1)         (r1 is a loop)
 *   b = c = y, a = x != y  m(x,y) (m(x,y)-1) s(y)         (r2 is a loop)
 *   a = c = x, b = y != x  m(x,y) m(y,x) s(x)             (r3 is a loop)
 *   a = b = c = x          s(x) (s(x)-1) (s(x)-2)
 * The count is the sum of all of these.  The pattern is not symmetric under rotation: the positions are three
 * roles, and a count grouped by a role credits each term to the node in that role (the b = c = y term goes to x
 * for the source and to y for the middle and the sink).  The three roles' counts have the same sum.
 * The _by_node forms follow the result contract of capsmi_trigraph_count_by_node: two non-nullable Long columns,
 * the graph's own ids and the counts, one row per node with a non-zero count, in no particular order.  Single
 * device: a trigraph of a distributed build gives CAPSMI_ERR_UNSUPPORTED; a role outside 0..2 gives
 * CAPSMI_ERR_ILLEGAL_ARGUMENT. */
enum { CAPSMI_TRI_ROLE_SOURCE = 0, CAPSMI_TRI_ROLE_MIDDLE = 1, CAPSMI_TRI_ROLE_SINK = 2 }; /* a, b, c */
capsmi_status capsmi_trigraph_count_transitive(capsmi_session* s, const capsmi_trigraph* g, int64_t* out_rows);
capsmi_status capsmi_trigraph_count_transitive_by_node(capsmi_session* s, const capsmi_trigraph* g, int32_t role,
                                                       const char* id_name, const char* count_name,
                                                       capsmi_table** out);
capsmi_status capsmi_triangle_count_transitive(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                               const char* src_col, const char* dst_col, const capsmi_bitmap* n_ok,
                                               int64_t* out_rows);
capsmi_status capsmi_triangle_count_transitive_by_node(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                                       const char* src_col, const char* dst_col,
                                                       const capsmi_bitmap* n_ok, int32_t role, const char* id_name,
                                                       const char* count_name, capsmi_table** out);
/* The undirected triangle over the same trigraph, as RelationalPlanner plans it:
 *   MATCH (a)-[r1]-(b)-[r2]-(c)-[r3]-(a) WHERE n_ok(a) AND n_ok(b) AND n_ok(c) RETURN count(*)
 *   ... RETURN id(a), count(*)     (or id(b), or id(c))
 * Bindings are rows: r1, r2, r3 are pairwise distinct, node variables may coincide, and the one node filter
 * applies to all three positions.  The two Expands bind a self-loop once (their incoming branch runs over the
 * relationships with start <> end); the closing ExpandInto is a union of two joins without that filter and binds
 * a self-loop twice.  With m(x,y) the multiplicity of x->y for x != y, s(x) the self-loops at x,
 * U(x,y) = m(x,y) + m(y,x) and Q(x,y) = U(x,y) (U(x,y) - 1), the bindings split by how many of a, b, c coincide:
 *   three distinct nodes   U(a,b) U(b,c) U(c,a) per ordered triple; a simple triangle {x,y,z} gives 6 U U U in
 *                          all, and 2 U U U to each corner at each position
 *   a = b = x, c = y != x  s(x) Q(x,y)                     (r1 is a loop)
 *   b = c = y, a = x != y  Q(x,y) s(y)                     (r2 is a loop)
 *   a = c = x, b = y != x  2 s(x) Q(x,y)                   (r3 is a loop, bound twice)
 *   a = b = c = x          2 s(x) (s(x)-1) (s(x)-2)
 * The count is the sum of all of these.  The closing hop makes the positions two classes: the ends of the
 * ExpandInto (a and c give the same rows: CAPSMI_TRI_UND_END) and the middle b (CAPSMI_TRI_UND_MIDDLE).  With
 * T(x) = sum over y, z of U(x,y) U(y,z) U(z,x):
 *   end(x)    = T(x) + sum_y [3 s(x) + s(y)] Q(x,y) + 2 s(x) (s(x)-1) (s(x)-2)
 *   middle(x) = T(x) + sum_y [2 s(x) + 2 s(y)] Q(x,y) + 2 s(x) (s(x)-1) (s(x)-2)
 * and both classes' counts sum to the count.  The _by_node forms follow the result contract of
 * capsmi_trigraph_count_by_node: two non-nullable Long columns, the graph's own ids and the counts, one row per
 * node with a non-zero count, in no particular order.  Single device: a trigraph of a distributed build gives
 * CAPSMI_ERR_UNSUPPORTED; a position outside 0..1 gives CAPSMI_ERR_ILLEGAL_ARGUMENT.  Config
 * CAPSMI_TRI_UND_COUNT = hash | walk selects the count's kernels (the same value either way). */
enum { CAPSMI_TRI_UND_END = 0, CAPSMI_TRI_UND_MIDDLE = 1 }; /* a or c; b */
capsmi_status capsmi_trigraph_count_undirected(capsmi_session* s, const capsmi_trigraph* g, int64_t* out_rows);
capsmi_status capsmi_trigraph_count_undirected_by_node(capsmi_session* s, const capsmi_trigraph* g, int32_t position,
                                                       const char* id_name, const char* count_name,
                                                       capsmi_table** out);
capsmi_status capsmi_triangle_count_undirected(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                               const char* src_col, const char* dst_col, const capsmi_bitmap* n_ok,
                                               int64_t* out_rows);
capsmi_status capsmi_triangle_count_undirected_by_node(capsmi_session* s, int32_t nrels, capsmi_table* const* rels,
                                                       const char* src_col, const char* dst_col,
                                                       const capsmi_bitmap* n_ok, int32_t position, const char* id_name,
                                                       const char* count_name, capsmi_table** out);
/* count(*) of the 2-hop chain (capsmi_two_hop_count) on one rank of an owner(target) partition:
 * this rank's tables hold every relationship into its owned ids [own_lo, own_hi) (relative to the
 * bitmaps' lo).  begin partitions them and writes the owned ids' in-degrees inA (relationships from
 * a_ok sources, b_ok applied) to owned_in (device, own_hi - own_lo uint32), stream-ordered; the
 * caller all-gathers the owned slices into one array of every id's inA, and finish sums inA(b) over
 * this rank's relationships b -> y with c_ok(y), less its a/b/c-ok self-loops, into *dev_out (device
 * int64, stream-ordered): the all-reduced sum of the ranks' parts is the count.  Σ_b inA(b)·outC(b)
 * (RelationalPlanner.scala:113-177 join rows, closed form in DESIGN.md §4) */
typedef struct capsmi_count_shard capsmi_count_shard;
capsmi_status capsmi_count_shard_begin(capsmi_session* s, int32_t nrels, capsmi_table* const* rels, const char* src_col,
                                       const char* dst_col, const capsmi_bitmap* a_ok, const capsmi_bitmap* b_ok,
                                       const capsmi_bitmap* c_ok, int64_t own_lo, int64_t own_hi, uint32_t* owned_in,
                                       capsmi_count_shard** out);
/* finish runs once per handle (a second call is ILLEGAL_ARGUMENT); the handle keeps what it reads of
 * the bitmaps, so they may be released after begin */
capsmi_status capsmi_count_shard_finish(capsmi_count_shard* h, const uint32_t* in_all, int64_t* dev_out);
capsmi_status capsmi_count_shard_release(capsmi_count_shard* h);
/* popcount of words [w_begin, w_end) of a device bitmap, result in *out (host) */
capsmi_status capsmi_words_popcount(capsmi_session* s, const uint32_t* words, int64_t w_begin, int64_t w_end,
                                    int64_t* out);
/* the same into a device int64 (*dev_out, overwritten), stream-ordered, no host synchronisation (the
 * count feeds a collective directly) */
capsmi_status capsmi_words_popcount_device(capsmi_session* s, const uint32_t* words, int64_t w_begin, int64_t w_end,
                                           int64_t* dev_out);

/* Cache analogue (Table.cache -> DataFrameTable.cache, SparkTable.scala:240-246): a copy of a
 * relationship table with rows clustered by `key_col` (dense ids in [id_lo, id_hi)).  Row multiset
 * unchanged; the fused kernels then touch bitmaps in id order. */
capsmi_status capsmi_cluster_by(capsmi_table* rels, const char* key_col, int64_t id_lo, int64_t id_hi,
                                capsmi_table** out);

/* ---- multi-GPU: one process per GPU over a distributed graph -------------------
 * Spark runs each Table operator over partitions and inserts a hash Exchange before joins and
 * aggregations (SparkTable.scala:133, 226; partitions set in CAPSSession.scala:115-131).  Here every
 * rank runs the same query (the same Table[T] calls) over its shard of a distributed graph; the fused
 * routes call the host's collective at their exchange points, so one rank's materialisation is one
 * rank's share of the job and the collective completes the answer on every rank.
 *
 * Ownership (hash partitioning): ids of the graph's domain [id_lo, id_hi) are scrambled by the
 * bijection h(x) = ((x - id_lo) * 0x9E3779B97F4A7C15) mod 2^k (2^k >= id_hi - id_lo, k >= 5) and rank
 * r owns the h-range [r * 32 * S, (r + 1) * 32 * S), S = ceil(2^k / (32 * world)) words -- balanced
 * whatever the id order (hubs at small ids included); the fused kernels run on h(x).
 *
 * The collective: enqueue one collective on the session's stream, ordered after the work queued on it
 * and before the work queued after the call returns (e.g. torch.distributed / RCCL on that stream).
 * ALL_GATHER: `count` elements from every rank into recv, rank-major (world x count);
 * ALL_REDUCE_SUM / _MAX: `count` elements, send and recv may be equal;
 * ALL_TO_ALL_V (Spark's Exchange hashpartitioning, SparkTable.scala:133, 226): `send` and `recv` point to
 * host capsmi_coll_vec descriptors and `count` is the world size; this rank sends send->counts[q]
 * elements, the q-th rank-major segment of send->data, to rank q and receives recv->counts[q] elements
 * from rank q into the q-th segment of recv->data (the library has exchanged the counts beforehand with
 * an ALL_GATHER, so both lists agree across ranks).  dtype CAPSMI_I64 (int64) or CAPSMI_COLL_U32
 * (uint32 words).  No call moves more than CAPSMI_COLL_CHUNK elements in all (environment, default
 * 2^26): the library cuts larger all-gathers, all-reduces and exchanges into several calls itself, so a
 * transport maps each call to one collective.  Return 0 on success. */
enum { CAPSMI_COLL_ALL_GATHER = 0, CAPSMI_COLL_ALL_REDUCE_SUM = 1, CAPSMI_COLL_ALL_REDUCE_MAX = 2,
       CAPSMI_COLL_ALL_TO_ALL_V = 3 };
enum { CAPSMI_COLL_U32 = 100 };
typedef struct {
    void* data;             /* device buffer, rank-major segments */
    const int64_t* counts;  /* host, world entries (elements per rank) */
} capsmi_coll_vec;
typedef int32_t (*capsmi_collective_fn)(void* ctx, int32_t op, const void* send, void* recv, int64_t count,
                                        int32_t dtype);
/* this process is rank `rank` of `world`; fn may be NULL only for world == 1 */
capsmi_status capsmi_session_set_ranks(capsmi_session* s, int32_t rank, int32_t world, capsmi_collective_fn fn,
                                       void* ctx);
enum { CAPSMI_NODES_REPLICATED = 0, CAPSMI_NODES_OWNED = 1 };
enum { CAPSMI_RELS_BY_SOURCE = 0, CAPSMI_RELS_BY_TARGET = 1 };
/* Registers this rank's entity tables (capsmi_node_table / capsmi_rel_table) as its shard of a graph
 * over the id domain [id_lo, id_hi) (the same on every rank, covering every id; hi - lo <= 2^30):
 * node tables hold every node row (REPLICATED) or the rows of the ids this rank owns (OWNED);
 * relationship tables hold the relationships whose target (BY_TARGET) or source (BY_SOURCE) this rank
 * owns.  Checked: ids inside the domain and the shard's rows owned (else ILLEGAL_ARGUMENT).  The
 * tables keep their scrambled key columns.  With BY_SOURCE, registration also exchanges (ALL_TO_ALL_V)
 * every relationship whose target another rank owns to that rank, which keeps it as its shard's
 * in-relationships (the var-length and undirected routes need them).  Routed on a distributed graph:
 * Expand projections (rows of this rank's relationships) and count(*) (one SUM all-reduce); either mode:
 * the 2-hop count(*), count(DISTINCT end) and count(DISTINCT start) (all-gathers of owned frontier slices
 * when the walk's relationships arrive by their end's owner, an ALL_TO_ALL_V + OR of frontier and end
 * bitmap slices when by their start's owner; the count(*) through an all-gather of owned degrees) and the
 * cyclic triangle count (sampled degrees all-reduced, every relationship packed into its oriented key and
 * exchanged to the rank of its source's degree-order range, sorted and deduplicated there, the ranges
 * all-gathered into a replicated oriented graph, each rank counting an interleaved share of the centers, one
 * all-reduce); with BY_SOURCE also the var-length grouped count (od and Y all-reduced
 * between its phases; the rows of each rank's owned start nodes), the undirected 1- / 2-hop counts (the
 * middles restricted to owned ids over the relationships incident to them, marks OR-reduced) and the 2-hop
 * grouped by its start (outC and the deduplicated hop-2 lists all-gathered; rows of the owned starts).
 * Any other plan runs operator by operator with the Exchanges Spark would insert (hash-partitioned joins
 * and groupings, gathers for global aggregates and ordering); capsmi_table_partitioned tells which results
 * hold this rank's rows only.  A session given a collective at world size 1 runs the same
 * distributed routes over its single shard (every exchange then goes through the collective). */
capsmi_status capsmi_graph_distribute(capsmi_session* s, int64_t id_lo, int64_t id_hi, int32_t nnodes,
                                      capsmi_table* const* nodes, int32_t node_mode, int32_t nrels,
                                      capsmi_table* const* rels, int32_t rel_mode);
/* the rows of `t` whose Long column `col` holds an id this rank owns in [id_lo, id_hi) (ingest: a
 * rank keeps its shard of a table every rank read); a new materialised table */
capsmi_status capsmi_owned_rows(capsmi_session* s, capsmi_table* t, const char* col, int64_t id_lo, int64_t id_hi,
                                capsmi_table** out);
/* the rank owning Long id `id` of the domain [id_lo, id_hi) among `world` ranks, and its scrambled
 * dense id (host computation, no device) */
capsmi_status capsmi_id_owner(int64_t id_lo, int64_t id_hi, int32_t world, int64_t id, int32_t* owner,
                              int64_t* dense_id);
/* 1 when t's rows are this rank's partition of a distributed result, else 0 (materialises t) */
capsmi_status capsmi_table_partitioned(const capsmi_table* t, int32_t* out);

/* ---- synthetic input -----------------------------------------------------
 * R-MAT relationship table [id, source, target] generated on the device, identical edge for edge
 * to oracle/rmat.c.  Keeps edges e in [e_begin, e_end) whose `part_col` (0 = source, 1 = target,
 * -1 = no filter) id falls in the word-aligned owner range of part `part` of `nparts`. */
capsmi_status capsmi_rmat_rels(capsmi_session* s, int32_t scale, int64_t e_begin, int64_t e_end,
                               int32_t pa, int32_t pb, int32_t pc, uint64_t seed, int32_t part_col,
                               int32_t part, int32_t nparts, capsmi_table** out);
/* word range [w_begin, w_end) of part `part` of `nparts` for ids in [0, 2^scale) */
capsmi_status capsmi_owner_words(int64_t nbits, int32_t part, int32_t nparts, int64_t* w_begin,
                                 int64_t* w_end);
/* ---- ingest ----------------------------------------------------
 * DataFrameReader.csv with an explicit schema, as EdgeListDataSource (EdgeListDataSource.scala:76-97)
 * and the FS graph source read their tables: files in order, no header, `delimiter` one character
 * (as Spark's `sep`: "1  2" with ' ' is 1, null, 2; 0 = opt-in whitespace splitting, runs of blanks
 * separate fields), '"' quotes, an empty unquoted field is null, lines whose first character is
 * `comment` (0 = none) and lines of blanks skipped; Spark's PERMISSIVE token counts (missing trailing fields null, extra tokens dropped);
 * a token that does not parse as its column type is ILLEGAL_ARGUMENT.  Parsed by host threads
 * (CAPSMI_INGEST_THREADS, default OMP_NUM_THREADS), copied to the device.  types: CAPSMI_I64 /
 * F64 / BOOL / STR; STR fields go through `intern` (the caller's dictionary), in row order.
 * row_id_col != NULL prepends a Long column of monotonically_increasing_id values
 * (EdgeListDataSource.scala:86): by default those of one partition (the row numbers); see
 * capsmi_session_set_csv_partitioning for Spark's multi-partition ids. */
typedef int64_t (*capsmi_intern_fn)(void* ctx, const char* s, size_t len);
/* Row ids of capsmi_read_csv as monotonically_increasing_id over the partitions of Spark 2.2.1's file scan
 * (FileSourceScanExec.createNonBucketedReadRDD; third-party, restated in csrc/ingest.hip spark_row_ids):
 * maxSplitBytes = min(max_partition_bytes, max(open_cost_bytes, total / default_parallelism)), total =
 * sum of (file length + open_cost_bytes); files split every maxSplitBytes; splits sorted by length
 * (descending, stable) and packed next-fit into partitions; a line belongs to the split holding the byte
 * before its first byte (Hadoop's LineRecordReader); id = partition << 33 | row within the partition.
 * default_parallelism = the session's core count (CAPSSession.local(): local[*]); 0 restores one partition.
 * Spark's defaults: max_partition_bytes 128 MiB (spark.sql.files.maxPartitionBytes), open_cost_bytes 4 MiB
 * (spark.sql.files.openCostInBytes). */
capsmi_status capsmi_session_set_csv_partitioning(capsmi_session* s, int64_t default_parallelism,
                                                  int64_t max_partition_bytes, int64_t open_cost_bytes);
capsmi_status capsmi_read_csv(capsmi_session* s, int32_t nfiles, const char* const* paths, char delimiter, char comment,
                              int32_t ncols, const char* const* names, const int32_t* types, capsmi_intern_fn intern,
                              void* intern_ctx, const char* row_id_col, capsmi_table** out);

/* R-MAT node table(s): kind 0 -> one table [id] with every id 0..2^scale-1 (all Person);
 * kind 1 -> Person ids (splitmix64(id) & 3 != 0) with [id, age], age = splitmix64(seed ^ id) % 100;
 * kind 2 -> Company ids (the complement) with [id] */
capsmi_status capsmi_rmat_nodes(capsmi_session* s, int32_t scale, int32_t kind, uint64_t seed,
                                capsmi_table** out);
/* order-insensitive row fingerprint over `ncols` I64 columns (SURVEY.md §8d parity check):
 * count, sum and xor of h(row), h = fold splitmix64(h ^ v) from 0x243F6A8885A308D3 */
capsmi_status capsmi_table_fingerprint(capsmi_table* t, int32_t ncols, const char* const* cols,
                                       int64_t* count, uint64_t* sum, uint64_t* xr);

#ifdef __cplusplus
}
#endif
#endif /* CAPSMI_H */
